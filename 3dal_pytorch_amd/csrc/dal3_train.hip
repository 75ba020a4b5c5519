// dal3_train.hip — training-mode building blocks for the shared-MLP stacks: what
// `loss.backward()` drives through Conv1d(k=1) + BatchNorm1d(batch statistics) + ReLU + max over points in
// tools/static_model.py:271-295,326-339 (and the dynamic twins), as fp32 MFMA kernels over POINT-MAJOR row-major
// activations  a[M x C]  (M = B*N points; what `(B,C,N).transpose(2,1)` is in memory).
//
// Why row-major point-major: the same buffer feeds all three GEMM shapes of a layer without a transpose —
//   forward   z[M x Co]  = act(a)[M x Ci] . W^T         channels on MFMA rows, points on lanes: a lane reads four
//   dgrad     da[M x Ci] = dz[M x Co] . W               consecutive channels of ITS point (16 B), the accumulator
//                                                       tile stores the same way;
//   wgrad     dW[Co x Ci] = dz^T . act(a)               the contraction runs over POINTS: the A operand wants lane =
//                                                       out-channel, k = point, i.e. for each point 32 consecutive
//                                                       floats of a row: a 128-B coalesced row segment per half-wave.
// Train-mode BN needs the statistics of a layer's whole output before the next layer can run, so — unlike the
// eval kernels, which chain a tile through a whole network in registers — every layer's pre-BN output z is
// materialised once; normalisation + ReLU are applied on load by the consumer ("act": y = max(z*scale+shift, 0)).
// All channel counts are multiples of 32 here (the host pads 3 -> 32 input channels and 2 -> 32 logits; that is
// < 1 % of the work) and M is a multiple of 32.
#include <type_traits>

#include "dal3_block.h"
#include "dal3_device.h"
#include "dal3_kernels.h"

#define TR_T 2                          // point tiles (32 points each) per wave in the linear kernel
#define TR_MTB 4                        // output tiles (32 channels each) per wave: 4*2*16 = 128 accumulator registers
#define TR_MAX_ACT_CIN 1024              // most input channels of a layer whose input carries an activation

// ---------------------------------------------------------------------------------------------- linear
// z[p][co] (+)= sum_ci act(a[p][ci]) * Wop[co][ci] + bias
//   Wop = W (row-major (c_out, c_in), ldw = row stride)           when !transpose_w   (forward)
//   Wop[co][ci] = W[ci][co] with W row-major (c_in, c_out)         when  transpose_w   (dgrad: W is the layer's
//                                                                   (c_out_fwd, c_in_fwd) matrix, co here = ci_fwd)
//   act: scale == NULL -> identity; else y = z*scale[ci] + shift[ci], then max(y,0) if relu_in
//   bias: NULL, per-channel (seg == 0) or per-segment (bias[(p / seg) * c_out + co], the decoder's per-crop term)
// grid: (M/32/TR_T, c_out/32/TR_MTB rounded up); one wave per block of 64 threads x 4 waves? -> 1 wave = 1 unit.
// One k-tile (32 input channels) of operands for a wave: the activation tiles of its TR_T point tiles and the weight
// fragments of its TR_MTB output tiles. Two of these ping-pong: the loads of k-tile kt+1 are issued before the 128
// MFMAs of k-tile kt, so their L2 latency passes under the matrix work (hipcc left alone sinks each load to its
// first use; the sched_barrier between "load next" and "compute current" keeps them apart).
struct TrStage {
    f32x16 X[TR_T];
    f32x4 sc[4], sh[4];                 // the k-tile's per-channel affine for this lane's channel groups
    f32x4 Wf[TR_MTB][4];
};

// Loads only. The activation (affine + ReLU) is applied by tr_act_stage right before the stage is consumed: doing
// it here would make the wave wait for the data it has just requested, i.e. expose the full load latency per k-tile.
__device__ __forceinline__ void tr_load_stage(TrStage& st, int kt, const float* __restrict__ a, int64_t lda,
                                              const int64_t (&prow)[TR_T], const float* __restrict__ scale,
                                              const float* __restrict__ shift, const float* __restrict__ W,
                                              int64_t ldw, int transpose_w, int mt0, int n_mt, int h, int m) {
#pragma unroll
    for (int j = 0; j < TR_T; ++j) {
        const float* ap = a + prow[j] * lda + 32 * kt + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(ap + 8 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) st.X[j][4 * q + e] = v[e];
        }
    }
    if (scale) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            st.sc[q] = *reinterpret_cast<const f32x4*>(scale + 32 * kt + 8 * q + 4 * h);
            st.sh[q] = *reinterpret_cast<const f32x4*>(shift + 32 * kt + 8 * q + 4 * h);
        }
    }
#pragma unroll
    for (int t = 0; t < TR_MTB; ++t) {
        if (t >= n_mt) break;
        const int row = 32 * (mt0 + t) + m;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 32 * kt + 8 * q + 4 * h;
            if (!transpose_w) {
                st.Wf[t][q] = *reinterpret_cast<const f32x4*>(W + (int64_t)row * ldw + col);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) st.Wf[t][q][e] = W[(int64_t)(col + e) * ldw + row];
            }
        }
    }
}

__device__ __forceinline__ void tr_act(f32x16 (&X)[TR_T], const f32x4 (&sc)[4], const f32x4 (&sh)[4], bool act, int relu_in) {
    if (!act) return;
#pragma unroll
    for (int j = 0; j < TR_T; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = X[j][r] * sc[r >> 2][r & 3] + sh[r >> 2][r & 3];
            X[j][r] = relu_in ? fmaxf(v, 0.0f) : v;
        }
}

__device__ __forceinline__ void tr_compute_stage(const TrStage& st, f32x16 (&acc)[TR_T][TR_MTB], int n_mt) {
#pragma unroll
    for (int t = 0; t < TR_MTB; ++t) {
        if (t >= n_mt) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int j = 0; j < TR_T; ++j) acc[j][t] = mfma32(st.Wf[t][q][e], st.X[j][4 * q + e], acc[j][t]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void tr_linear_kernel(const float* __restrict__ a, int64_t M, int c_in, int64_t lda,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        int relu_in, const float* __restrict__ W, int64_t ldw,
                                                        int transpose_w, const float* __restrict__ bias, int64_t seg,
                                                        int c_out, float* __restrict__ z, int64_t ldz, int accumulate,
                                                        int n_mblk) {
    const int lane = threadIdx.x & 63, h = lane >> 5, m = lane & 31;
    const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar: so is everything derived from it)
    const int mblk = (int)(unit % n_mblk);
    const int64_t pt0 = (unit / n_mblk) * (32 * TR_T);
    if (pt0 >= M) return;
    const int mt0 = mblk * TR_MTB;
    const int n_mt = min(TR_MTB, c_out / 32 - mt0);
    const int KT = c_in / 32;
    int64_t prow[TR_T];
#pragma unroll
    for (int j = 0; j < TR_T; ++j) prow[j] = min(pt0 + 32 * j, M - 32) + m;     // a tile past the end recomputes the last one

    f32x16 acc[TR_T][TR_MTB];
#pragma unroll
    for (int j = 0; j < TR_T; ++j) {
#pragma unroll
        for (int t = 0; t < TR_MTB; ++t) {
            if (t < n_mt && bias) {
                const float* bp = bias + (seg > 0 ? (prow[j] / seg) * c_out : 0) + 32 * (mt0 + t);
                acc[j][t] = tile_from_channels(bp, h);
            } else {
                acc[j][t] = f32x16{};
            }
        }
    }
    // ping-pong over the k-tiles; the k index of a load past the end is clamped (valid memory, values unused) so that
    // no load sits behind a data-dependent branch, and only the matching compute is skipped
    TrStage s0, s1;
    tr_load_stage(s0, 0, a, lda, prow, scale, shift, W, ldw, transpose_w, mt0, n_mt, h, m);
    for (int kt = 0; kt < KT; kt += 2) {
        tr_load_stage(s1, min(kt + 1, KT - 1), a, lda, prow, scale, shift, W, ldw, transpose_w, mt0, n_mt, h, m);
        DAL3_SCHED_FENCE();
        tr_act(s0.X, s0.sc, s0.sh, scale != nullptr, relu_in);
        tr_compute_stage(s0, acc, n_mt);
        DAL3_SCHED_FENCE();
        tr_load_stage(s0, min(kt + 2, KT - 1), a, lda, prow, scale, shift, W, ldw, transpose_w, mt0, n_mt, h, m);
        DAL3_SCHED_FENCE();
        if (kt + 1 < KT) {
            tr_act(s1.X, s1.sc, s1.sh, scale != nullptr, relu_in);
            tr_compute_stage(s1, acc, n_mt);
        }
        DAL3_SCHED_FENCE();
    }
#pragma unroll
    for (int j = 0; j < TR_T; ++j) {
        if (pt0 + 32 * j >= M) break;
        float* zp = z + (pt0 + 32 * j + m) * ldz + 4 * h;
#pragma unroll
        for (int t = 0; t < TR_MTB; ++t) {
            if (t >= n_mt) break;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4* dst = reinterpret_cast<f32x4*>(zp + 32 * (mt0 + t) + 8 * q);
                f32x4 o = {acc[j][t][4 * q], acc[j][t][4 * q + 1], acc[j][t][4 * q + 2], acc[j][t][4 * q + 3]};
                if (accumulate) {
                    const f32x4 old = *dst;
                    o[0] += old[0];
                    o[1] += old[1];
                    o[2] += old[2];
                    o[3] += old[3];
                }
                *dst = o;
            }
        }
    }
}

// ---- fast path for c_out % 128 == 0 (every big layer): the weights are first re-ordered into MFMA fragment order
// ([output block][k-tile][tile][q] x 1 KiB, tr_pack_kernel: a few microseconds) so that a fragment is ONE coalesced
// 1-KiB load, and they are streamed through the 8-deep prefetch ring of the eval kernels (dal3_device.h) instead of
// being double-buffered per k-tile: 128 accumulator + 64 activation + 32 ring registers leave room for two waves per
// SIMD, so one wave's prologue/epilogue hides under the other's MFMAs.
__device__ __forceinline__ void tr_pack_element(const float* __restrict__ W, int64_t ldw, int transpose_w, int c_out, int c_in,
                                                int mtb, float* __restrict__ out, int64_t i) {
    if (i >= (int64_t)c_out * c_in) return;
    const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
    int64_t f = i >> 8;                                       // fragment index
    const int q = (int)(f & 3);
    f >>= 2;
    const int t = (int)(f % mtb);
    f /= mtb;
    const int KT = c_in / 32;
    const int kt = (int)(f % KT), mblk = (int)(f / KT);
    const int row = 32 * (mtb * mblk + t) + (lane & 31), col = 32 * kt + 8 * q + 4 * (lane >> 5) + e;
    out[i] = transpose_w ? W[(int64_t)col * ldw + row] : W[(int64_t)row * ldw + col];
}
// The f16x3 image of the same matrix (dal3_train_x3.hip; layout code 0x100 | MTB): per output block of MTB tiles one stream
// [k-tile][out-tile][k-step][hi | lo] of 1-KiB fp16 fragments (64 lanes x 8 values, k order as launch_pack_weight_lp),
// hi = fp16(w), lo = fp16(w - hi). i runs over c_out * c_in * 2 fp16 values: the same number of bytes as the fp32 image.
__device__ __forceinline__ void tr_pack_x3_element(const float* __restrict__ W, int64_t ldw, int transpose_w, int c_out, int c_in,
                                                   int mtb, uint16_t* __restrict__ out, int64_t i) {
    if (i >= (int64_t)c_out * c_in * 2) return;
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63), half = (int)((i >> 9) & 1), s = (int)((i >> 10) & 1);
    int64_t f = i >> 11;                                      // (out-tile, k-tile) block
    const int t = (int)(f % mtb);
    f /= mtb;
    const int KT = c_in / 32;
    const int kt = (int)(f % KT), mblk = (int)(f / KT);
    const int row = 32 * (mtb * mblk + t) + (lane & 31), col = 32 * kt + 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
    const float v = transpose_w ? W[(int64_t)col * ldw + row] : W[(int64_t)row * ldw + col];
    // (a weight beyond fp16's range — the f16x3 contract of dal3.h — becomes NaN, not a saturated value: every output of
    // the layer is then NaN, which a training loop and a test both notice)
    const _Float16 hi = fabsf(v) < 65504.0f ? (_Float16)v : (_Float16)__builtin_nanf("");
    const _Float16 lo = (_Float16)(v - (float)hi);
    out[i] = __builtin_bit_cast(uint16_t, half ? lo : hi);
}
__global__ void tr_pack_kernel(const float* __restrict__ W, int64_t ldw, int transpose_w, int c_out, int c_in, int mtb,
                               float* __restrict__ out) {
    tr_pack_element(W, ldw, transpose_w, c_out, c_in, mtb, out, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
static void tr_pack(const float* W, int64_t ldw, int transpose_w, int c_out, int c_in, int mtb, float* ws, hipStream_t s) {
    hipLaunchKernelGGL(tr_pack_kernel, dim3((unsigned)(((int64_t)c_out * c_in + 255) / 256)), dim3(256), 0, s, W, ldw, transpose_w, c_out,
                       c_in, mtb, ws);
}
// Every layer of a step packed by ONE launch (round 3: a training step issued 32 tr_pack launches of ~4 us, one in front
// of each linear / dgrad call; the weights do not change between a step's forward and its backward, so both orientations
// of every layer can be packed when the forward starts). The item table travels by value in the kernel arguments.
#define TR_PACK_MAX 48
struct TrPackItem {
    const float* W;
    float* out;
    int64_t ldw;
    int32_t transpose_w, c_out, c_in, mtb;
    uint32_t first_block;                                   // of 256 threads; blocks [first_block, next item's) belong to it
};
struct TrPackMany {
    TrPackItem it[TR_PACK_MAX];
    int n;
};
__global__ __launch_bounds__(256) void tr_pack_many_kernel(TrPackMany p) {
    int k = 0;
    for (int i = 1; i < p.n; ++i) k = blockIdx.x >= p.it[i].first_block ? i : k;      // (first_block is ascending)
    const TrPackItem& t = p.it[k];
    const int64_t i = (int64_t)(blockIdx.x - t.first_block) * 256 + threadIdx.x;
    if (t.mtb & 0x100)
        tr_pack_x3_element(t.W, t.ldw, t.transpose_w, t.c_out, t.c_in, t.mtb & 0xff, reinterpret_cast<uint16_t*>(t.out), i);
    else
        tr_pack_element(t.W, t.ldw, t.transpose_w, t.c_out, t.c_in, t.mtb, t.out, i);
}

template <int T>
struct TrX {
    f32x16 X[T];
};

// y = max(x*scale + shift, 0) with the per-channel affine read from LDS (copied there once per workgroup): keeping
// it in registers from load to use costs 32 VGPRs per stage and pushed the kernel into scratch
template <int T>
__device__ __forceinline__ void tr_act_lds(f32x16 (&X)[T], const float* __restrict__ s_sc, const float* __restrict__ s_sh,
                                           int kt, int h, int relu_in) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(s_sc + 32 * kt + 8 * q + 4 * h);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(s_sh + 32 * kt + 8 * q + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const float v = X[j][4 * q + e] * sc[e] + sh[e];
                X[j][4 * q + e] = relu_in ? fmaxf(v, 0.0f) : v;
            }
    }
}

// The input activation's scale and shift copied to LDS, once per workgroup of 256 threads (barrier included); false: the
// input carries no activation and nothing is staged.
__device__ __forceinline__ bool tr_stage_act(const float* __restrict__ scale, const float* __restrict__ shift, int c_in,
                                             float* __restrict__ s_sc, float* __restrict__ s_sh) {
    if (!scale) return false;
    for (int i = threadIdx.x; i < c_in; i += 256) {
        s_sc[i] = scale[i];
        s_sh[i] = shift[i];
    }
    __syncthreads();
    return true;
}

template <int T>
__device__ __forceinline__ void tr_load_x(TrX<T>& st, int kt, const float* __restrict__ a, int64_t lda,
                                          const int64_t (&prow)[T], int h) {
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const float* ap = a + prow[j] * lda + 32 * kt + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(ap + 8 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) st.X[j][4 * q + e] = v[e];
        }
    }
}

// the 4 MTB fragments (MTB output tiles x 4 q) of one k-tile, taken from the ring; BASE: the ring slot of the first
// (0, or 4 for the second k-tile of a pair when a k-tile is only four fragments)
struct TrNoSide {
    __device__ __forceinline__ void operator()(int) const {}
};
// SWAP: the operands exchanged — the accumulator tile comes out TRANSPOSED (lane = output channel 32 t + m, register r =
// point 8 (r / 4) + 4 h + r % 4 of the tile): what a reduction over the points wants (sums over registers, no cross-lane
// work), and its stores are whole 128-byte rows. The fragments themselves are the same (lane (m, h) of a weight fragment
// holds row m, k = h; of an activation fragment point m, k = h: either can be the A or the B operand).
template <int T, int MTB, int BASE, bool SWAP = false, class Ring, class Side = TrNoSide>
__device__ __forceinline__ void tr_ring_block(Ring& ring, const f32x16 (&X)[T], f32x16 (&acc)[T][MTB], Side side = Side()) {
#pragma unroll
    for (int i = 0; i < 4 * MTB; ++i) {
        const f32x4 w = ring.slot[(BASE + i) % DAL3_PF];
        ring.slot[(BASE + i) % DAL3_PF] = ring.fetch();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int j = 0; j < T; ++j)
                acc[j][i / 4] = SWAP ? mfma32(X[j][4 * (i % 4) + e], w[e], acc[j][i / 4]) : mfma32(w[e], X[j][4 * (i % 4) + e], acc[j][i / 4]);
        }
        DAL3_SCHED_FENCE();
        side(i);
    }
}

// T point tiles x MTB output tiles per wave. <2, 4>: the big layers (c_out % 128 == 0). <2, 2>: c_out % 64 == 0 (the
// 64-channel layers and their gradients; through the strided-weight kernel above the 512 -> 64 dgrad of dconv1 ran at
// 65 TFLOP/s). <1, 1>: few rows (the per-item FC tails: 64 rows x 512 channels as <2, 4> is FOUR waves walking K = 512
// one after the other, 83 us; as 32 waves of one tile each, a fraction of that).
#ifndef TR_RING_OCC
#define TR_RING_OCC 1                   // waves per SIMD the kernel is compiled for: at 2 (256 registers) <2, 4> spilled and ran 5 % slower
#endif
template <int T, int MTB, int OCC>
__global__ __launch_bounds__(256, OCC) void tr_linear_ring_kernel(const float* __restrict__ a, int64_t M, int c_in, int64_t lda,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift, int relu_in,
                                                                const f32x4* __restrict__ wpk, const float* __restrict__ bias,
                                                                int64_t seg, int c_out, float* __restrict__ z, int64_t ldz,
                                                                int accumulate, int n_mblk) {
    static_assert(DAL3_PF == 8 && (MTB == 1 || MTB == 2 || MTB == 4), "fragment order of tr_pack_kernel, ring slots");
    __shared__ float s_sc[TR_MAX_ACT_CIN], s_sh[TR_MAX_ACT_CIN];
    const bool act = tr_stage_act(scale, shift, c_in, s_sc, s_sh);
    const int lane = threadIdx.x & 63, h = lane >> 5, m = lane & 31;
    // scalar (the ring's buffer descriptor stays in SGPRs: from a per-lane value hipcc builds a waterfall loop around every
    // fragment fetch) and 32-bit (a 64-bit division is ~200 instructions; the host keeps the unit count below 2^32)
    const uint32_t unit = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int mblk = (int)(unit % (uint32_t)n_mblk);
    const int64_t pt0 = (int64_t)(unit / (uint32_t)n_mblk) * (32 * T);
    if (pt0 >= M) return;
    const int mt0 = mblk * MTB;
    const int KT = c_in / 32;
    int64_t prow[T];
#pragma unroll
    for (int j = 0; j < T; ++j) prow[j] = min(pt0 + 32 * j, M - 32) + m;
    WRing<DAL3_PF> ring;
    ring.init(wpk + (int64_t)mblk * KT * (4 * MTB) * 64, lane);
    f32x16 acc[T][MTB];
    if (bias) {
#pragma unroll
        for (int j = 0; j < T; ++j) {
            // the per-segment term's row: ONE division per point tile, scalar when a tile cannot straddle two segments
            // (seg % 32 == 0: every caller with N % 32 == 0), 32-bit per lane otherwise — `prow[j] / seg` as written, a
            // 64-bit division per lane and output tile, was ~1,000 of the 1,400 vector instructions in front of the
            // first MFMA (4 us per wave against 7 us of MFMAs for a K = 64 layer)
            int64_t row = 0;
            if (seg > 0) {
                const int64_t first = min(pt0 + 32 * j, M - 32);
                row = (seg % 32 == 0) ? (int64_t)((uint32_t)first / (uint32_t)seg) : (int64_t)((uint32_t)prow[j] / (uint32_t)seg);
            }
            const float* bp = bias + row * c_out + 32 * mt0;
#pragma unroll
            for (int t = 0; t < MTB; ++t) acc[j][t] = tile_from_channels(bp + 32 * t, h);
        }
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int t = 0; t < MTB; ++t) acc[j][t] = f32x16{};
    }
    constexpr int BASE2 = (4 * MTB) % DAL3_PF;               // ring slot of the second k-tile's first fragment
    TrX<T> xa, xb;                                           // raw loads one k-tile ahead; activation applied at use
    tr_load_x<T>(xa, 0, a, lda, prow, h);
    for (int kt = 0; kt < KT; kt += 2) {
        tr_load_x<T>(xb, min(kt + 1, KT - 1), a, lda, prow, h);
        DAL3_SCHED_FENCE();
        if (act) tr_act_lds<T>(xa.X, s_sc, s_sh, kt, h, relu_in);
        tr_ring_block<T, MTB, 0>(ring, xa.X, acc);
        tr_load_x<T>(xa, min(kt + 2, KT - 1), a, lda, prow, h);
        DAL3_SCHED_FENCE();
        if (kt + 1 < KT) {
            if (act) tr_act_lds<T>(xb.X, s_sc, s_sh, kt + 1, h, relu_in);
            tr_ring_block<T, MTB, BASE2>(ring, xb.X, acc);
        }
    }
    // (the branch on `accumulate` OUTSIDE the store loops: inside, it is a branch per store — 64 per wave)
    auto store_tiles = [&](auto acc_flag) {
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (pt0 + 32 * j >= M) break;
            float* zp = z + (pt0 + 32 * j + m) * ldz + 4 * h;
#pragma unroll
            for (int t = 0; t < MTB; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4* dst = reinterpret_cast<f32x4*>(zp + 32 * (mt0 + t) + 8 * q);
                    f32x4 o = {acc[j][t][4 * q], acc[j][t][4 * q + 1], acc[j][t][4 * q + 2], acc[j][t][4 * q + 3]};
                    if (decltype(acc_flag)::value) {
                        const f32x4 old = *dst;
                        o[0] += old[0];
                        o[1] += old[1];
                        o[2] += old[2];
                        o[3] += old[3];
                    }
                    *dst = o;
                }
            }
        }
    };
    if (accumulate)
        store_tiles(std::true_type{});
    else
        store_tiles(std::false_type{});
}

// The same layer with PERSISTENT waves (one workgroup per wave slot of the chip, each wave walking units wave, wave +
// n_waves, ...: a fixed output block, successive point tiles). Ablations of the kernel above (64 -> 512 at 262,144 rows:
// 269 us; without its stores 195, without its activation loads 213, without both 151 = its MFMAs) showed the three
// phases of a wave's life ADDING UP: workgroups that start together stay in step, so a CU loads, then multiplies, then
// stores. Here the phases of consecutive units overlap inside one wave: the first k-tile (and the bias row) of unit
// u + 1 are fetched BEFORE unit u's stores are issued (vmcnt counts loads and stores in issue order on gfx9: a load
// issued behind the stores could only be waited for together with them), the stores drain under unit u + 1's MFMAs
// (their data registers are read at issue), and the weight ring runs on cyclically (no refill bubble per unit).
// Host-side conditions (launch_tr_linear): no accumulate, M % (32 T) == 0, seg == 0 or seg % (32 T) == 0 (one bias row per
// unit), c_in % 64 == 0 (k-tiles in pairs; the ring's slot rotation is a compile-time pattern), n_waves % n_mblk == 0.
// The weight ring is the eval kernels' cyclic one (WRing<DAL3_PF, true> of dal3_device.h).

// RED != 0: a column reduction over the points of the kernel's OWN OUTPUT, taken in the epilogue instead of by a second
// pass over the tensor (round 4: the statistics / BatchNorm-backward passes were 1.0 of a training step's 7.9 ms, each a
// full read of a tensor the producing kernel had in registers a moment before):
//   RED == 1  sum z, sum z^2 of the output z                                   (dal3_tr_colred mode 0: batch statistics)
//   RED == 2  the output is da, the gradient w.r.t. relu(bn(bz)) of the layer whose pre-BN output is `bz`:
//             dy = da * [bz*bscale + bshift > 0];  sum dy, sum dy * (bz - bmu)*brstd    (mode 1: dbeta, dgamma)
// The tile is computed transposed (tr_ring_block SWAP): a lane owns ONE output channel of each tile and sixteen points of
// it, so the sums run over registers; a wave's units all lie in one channel block, so the running sums (float64) stay
// in registers for the wave's whole life and are written once: part[wave of the block][c][2], added in wave order by
// tr_colred_final_kernel. Fixed unit -> wave map, fixed order of additions: deterministic. NOT the separate pass's
// arithmetic in one respect: RED == 2 adds a tile's 16 T terms in fp32 before they join the float64 sums (see there;
// dal3.h states the bound), RED == 1 converts every term to float64 first like the separate pass.
struct TrRed {
    double* part;
    const float* bz;                     // RED == 2
    int64_t ldbz;
    const float* bscale;
    const float* bshift;
    const float* bmu;
    const float* brstd;
};

template <int T, int MTB, int OCC, int KTC, int RED = 0>     // KTC: c_in / 32 when it is 2 or 4 (straight-line code per unit), else 0
__global__ __launch_bounds__(256, OCC) void tr_linear_pers_kernel(const float* __restrict__ a, int64_t M, int c_in, int64_t lda,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift, int relu_in,
                                                                const f32x4* __restrict__ wpk, const float* __restrict__ bias,
                                                                int64_t seg, int c_out, float* __restrict__ z, int64_t ldz,
                                                                int n_mblk, uint32_t n_units, TrRed red) {
    static_assert(DAL3_PF == 8 && (MTB == 1 || MTB == 2 || MTB == 4), "fragment order of tr_pack_kernel, ring slots");
    // Every instantiation computes its tile TRANSPOSED (tr_ring_block SWAP), reduction or not: the stores are whole 128-byte
    // rows (measured against the untransposed tile: profiles/LEDGER_r04.md 2.1 item 2).
    __shared__ float s_sc[TR_MAX_ACT_CIN], s_sh[TR_MAX_ACT_CIN];
    const bool act = tr_stage_act(scale, shift, c_in, s_sc, s_sh);
    const int lane = threadIdx.x & 63, h = lane >> 5, m = lane & 31;
    uint32_t unit = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wave0 = unit;                              // this wave's index on the chip
    const uint32_t n_waves = gridDim.x * 4u;
    if (unit >= n_units) return;
    const int mblk = (int)(unit % (uint32_t)n_mblk);          // the same for every unit of this wave
    const int mt0 = mblk * MTB;
    const int KT = KTC ? KTC : c_in / 32;
    WRing<DAL3_PF, true> ring;
    ring.init(wpk + (int64_t)mblk * KT * (4 * MTB) * 64, lane, (uint32_t)(KT * 4 * MTB) * 1024u);
    auto bias_row = [&](int64_t pt0) {                        // scalar: one 32-bit division per unit
        return seg > 0 ? bias + (int64_t)((uint32_t)pt0 / (uint32_t)seg) * c_out + 32 * mt0 : bias + 32 * mt0;
    };
    auto bias_tile = [&](int64_t pt0, int t) {
        if (!bias) return f32x16{};
        const float v = bias_row(pt0)[32 * t + m];            // transposed tile: this lane's one channel in every register
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = v;
        return o;
    };
    int64_t pt0 = (int64_t)(unit / (uint32_t)n_mblk) * (32 * T);
    f32x16 bnext[MTB];
#pragma unroll
    for (int t = 0; t < MTB; ++t) bnext[t] = bias_tile(pt0, t);
    int64_t prow[T];
#pragma unroll
    for (int j = 0; j < T; ++j) prow[j] = pt0 + 32 * j + m;
    constexpr int BASE2 = (4 * MTB) % DAL3_PF;
    // RED: this lane's running sums per output tile, and (RED == 2) its channel's BatchNorm constants
    double r0[MTB], r1[MTB];
    float bsc[MTB], bsh[MTB], bmu[MTB], brs[MTB];
    if constexpr (RED != 0) {
#pragma unroll
        for (int t = 0; t < MTB; ++t) {
            r0[t] = 0.0;
            r1[t] = 0.0;
            if constexpr (RED == 2) {
                const int c = 32 * (mt0 + t) + m;
                bsc[t] = red.bscale[c];
                bsh[t] = red.bshift[c];
                bmu[t] = red.bmu[c];
                brs[t] = red.brstd[c];
            }
        }
    }
    // this lane's place inside a transposed tile, in bytes: row 4 h, column m (the host keeps 64 rows of either tensor below 2^31 bytes)
    const uint32_t loff_z = ((uint32_t)(4 * h) * (uint32_t)ldz + (uint32_t)m) * 4u;
    const uint32_t loff_bz = RED == 2 ? ((uint32_t)(4 * h) * (uint32_t)red.ldbz + (uint32_t)m) * 4u : 0u;
    TrX<T> xa, xb;
    tr_load_x<T>(xa, 0, a, lda, prow, h);
    // everything fetched so far has landed before the loop is entered: hipcc's wait-count pass merges the state at the
    // loop header from both edges, and with loads still pending on the entry edge it put an s_waitcnt vmcnt(8) at the top
    // of EVERY unit — i.e. a wait for the stores the previous unit had just issued (269 -> 248 us instead of -> 190)
    __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0) only (gfx9 encoding)
    for (;;) {
        f32x16 acc[T][MTB];
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int t = 0; t < MTB; ++t) acc[j][t] = bnext[t];
        const uint32_t unit_n = unit + n_waves;
        const bool more = unit_n < n_units;
        const int64_t pt0_n = more ? (int64_t)(unit_n / (uint32_t)n_mblk) * (32 * T) : pt0;
        int64_t prow_n[T];
#pragma unroll
        for (int j = 0; j < T; ++j) prow_n[j] = pt0_n + 32 * j + m;
        if (bias && seg > 0) {                                  // the next unit's bias row: waited for at the next unit's top
#pragma unroll
            for (int t = 0; t < MTB; ++t) bnext[t] = bias_tile(pt0_n, t);
        }
        // (scalar: the unit's first row of z / bz)
        const __amdgpu_buffer_rsrc_t zrs = __builtin_amdgcn_make_buffer_rsrc(z + pt0 * ldz, 0, 0x7fffffff, 0x00020000);
        __amdgpu_buffer_rsrc_t bzrs;
        if constexpr (RED == 2) bzrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(red.bz) + pt0 * red.ldbz, 0, 0x7fffffff, 0x00020000);
        // RED == 2: the tile of bz under output tile t (the same rows and channels, the transposed tile's own pattern: two
        // whole 128-byte rows per instruction), requested one output tile ahead of its use
        f32x16 bzt[2][T];
        auto load_bz = [&](int t) {
            if constexpr (RED == 2) {
#pragma unroll
                for (int j = 0; j < T; ++j) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        bzt[t & 1][j][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                            bzrs, loff_bz, (uint32_t)(((32 * j + (r & 3) + 8 * (r >> 2)) * (uint32_t)red.ldbz + 32 * (mt0 + t)) * 4u), 0));
                }
            }
        };
        // an output tile's stores go out as soon as its last MFMA has been issued (tile t: after fragment 4 t + 3 of the
        // LAST k-tile), between the MFMAs of the tiles behind it: issued in one burst at the end of the unit, the
        // 16 * T * MTB KiB of the workgroup's four waves queue up in front of the CU's one path to L2 and every wave
        // sits at its last store with the matrix pipe idle (ablation: 60 of the 215 us of 64 -> 512)
        auto store_tile = [&](int t) {
#pragma unroll
            for (int j = 0; j < T; ++j) {
                // through a buffer descriptor based at the unit's first row: the address of every store is that base +
                // ONE per-lane offset register + a scalar offset (with flat pointers hipcc keeps a 64-bit VGPR pair
                // per store in flight: 64 registers for a tile pair, and the kernel spilled)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[j][t][r]), zrs, loff_z,   // (not __builtin_bit_cast: on a vector ELEMENT it read element 0)
                                                          (uint32_t)(((32 * j + (r & 3) + 8 * (r >> 2)) * (uint32_t)ldz + 32 * (mt0 + t)) * 4u), 0);
            }
        };
        auto reduce_tile = [&](int t) {                         // (float64 per element, as the separate pass adds them)
            if constexpr (RED == 1) {
#pragma unroll
                for (int j = 0; j < T; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const double v = (double)acc[j][t][r];
                        r0[t] += v;
                        r1[t] = __builtin_fma(v, v, r1[t]);
                    }
            } else if constexpr (RED == 2) {
                // the tile's 16 T values per lane are summed in fp32 (two chains per sum), the tile sums join the float64
                // running sums: per element 7 fp32 operations instead of 5 + two conversions + two float64 operations,
                // which the matrix pipe had to wait for (256 -> 512: 0.66 -> see profiles/LEDGER_r04.md). These sums
                // have no variance-type cancellation; a 32-term fp32 partial sum is exact to ~1e-7 of its terms.
                float p0[2] = {0.0f, 0.0f}, p1[2] = {0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < T; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float zz = bzt[t & 1][j][r];
                        const float y = zz * bsc[t] + bsh[t];
                        const float dy = y > 0.0f ? acc[j][t][r] : 0.0f;
                        p0[r & 1] += dy;
                        p1[r & 1] = __builtin_fmaf(dy, (zz - bmu[t]) * brs[t], p1[r & 1]);
                    }
                r0[t] += (double)(p0[0] + p0[1]);
                r1[t] += (double)(p1[0] + p1[1]);
            }
        };
        auto kstep = [&](int kt, auto last_c) {                 // k-tiles kt and kt + 1 (KT is even on this path)
            constexpr bool LAST = decltype(last_c)::value;
            tr_load_x<T>(xb, kt + 1, a, lda, prow, h);
            DAL3_SCHED_FENCE();
            if (act) tr_act_lds<T>(xa.X, s_sc, s_sh, kt, h, relu_in);
            if (LAST) load_bz(0);
            if (LAST)
                tr_ring_block<T, MTB, 0, true>(ring, xa.X, acc, [&](int i) {
                    if (i == 2 * MTB && MTB > 1) load_bz(1);       // (half a round later: the two requests do not queue up together)
                });
            else
                tr_ring_block<T, MTB, 0, true>(ring, xa.X, acc);
            // k-tile kt + 2 of this unit, or — in the last round — the NEXT unit's first k-tile, ahead of the stores
            tr_load_x<T>(xa, LAST ? 0 : kt + 2, a, lda, LAST ? prow_n : prow, h);
            DAL3_SCHED_FENCE();
            if (act) tr_act_lds<T>(xb.X, s_sc, s_sh, kt + 1, h, relu_in);
            if (LAST)
                tr_ring_block<T, MTB, BASE2, true>(ring, xb.X, acc, [&](int i) {
                    if (i % 4 == 3) {
                        store_tile(i / 4);
                        reduce_tile(i / 4);
                        if (i / 4 + 2 < MTB) load_bz(i / 4 + 2);   // two tiles ahead, into the buffer the reduction has just read
                    }
                });
            else
                tr_ring_block<T, MTB, BASE2, true>(ring, xb.X, acc);
        };
        // first and last round peeled (the same one when K = 64): hipcc's wait counts are per code location, and the
        // waits of a unit's first fragments — fetched before the previous unit's stores — must count those stores as
        // younger (vmcnt(39...63)); inside ONE loop body they get the steady-state count of the later rounds, which at
        // the top of a unit is a wait for the stores
        if constexpr (KTC == 2) {
            kstep(0, std::true_type{});
        } else if constexpr (KTC == 4) {
            kstep(0, std::false_type{});
            kstep(2, std::true_type{});
        } else {                                               // KT >= 4
            kstep(0, std::false_type{});
            for (int kt = 2; kt + 2 < KT; kt += 2) kstep(kt, std::false_type{});
            kstep(KT - 2, std::true_type{});
        }
        if (!more) break;
        unit = unit_n;
        pt0 = pt0_n;
#pragma unroll
        for (int j = 0; j < T; ++j) prow[j] = prow_n[j];
    }
    if constexpr (RED != 0) {
        // the two half-waves of a channel hold disjoint points: fold them, one partial row per wave
        double* row = red.part + ((int64_t)(wave0 / (uint32_t)n_mblk) * c_out + 32 * mt0 + m) * 2;
#pragma unroll
        for (int t = 0; t < MTB; ++t) {
            const double s0 = r0[t] + __shfl_xor(r0[t], 32, 64);
            const double s1 = r1[t] + __shfl_xor(r1[t], 32, 64);
            if (h == 0) {
                row[64 * t] = s0;
                row[64 * t + 1] = s1;
            }
        }
    }
}

// ---- the pooled layer's forward without its output tensor: conv (W, b) -> BN -> ReLU -> max over the points of each
// segment, for layers whose batch statistics are known BEFORE the layer runs (train.py obtains them from the second
// moments of the layer's input). Same ring / ping-pong structure as tr_linear_ring_kernel, but the MFMA operands are
// SWAPPED (D^T = act(a) . W^T: points on the accumulator's registers, channels on its lanes — the idiom of the eval
// kernels' max-pooled layers), so the max over a tile's 32 points is a compare chain over 16 registers plus one
// exchange between the lane halves, each carrying the point index (pool_candidate of dal3_device.h, which also defines
// the key and the tie rule). The MFMA computes the same k-ordered FMA chain per output element whichever operand is
// which, so z — and with it g and arg — are bit-identical to tr_linear + tr_segmax. Candidates of different tiles /
// waves meet in the packed 64-bit atomicMax of tr_segmax_kernel. z itself (1 GB for ins_seg's conv5 at 64 x 4096
// points) is never written. seg must be a multiple of 32 (a tile lies in one segment).
__global__ __launch_bounds__(256, 2) void tr_linear_pool_kernel(const float* __restrict__ a, int64_t M, int c_in, int64_t lda,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift, int relu_in,
                                                                const f32x4* __restrict__ wpk, const float* __restrict__ bias,
                                                                const float* __restrict__ out_scale,
                                                                const float* __restrict__ out_shift, int64_t seg, int c_out,
                                                                unsigned long long* __restrict__ packed, int n_mblk) {
    __shared__ float s_sc[TR_MAX_ACT_CIN], s_sh[TR_MAX_ACT_CIN];
    const bool act = tr_stage_act(scale, shift, c_in, s_sc, s_sh);
    const int lane = threadIdx.x & 63, h = lane >> 5, m = lane & 31;
    const uint32_t unit = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (scalar, 32-bit: see tr_linear_ring_kernel)
    const int mblk = (int)(unit % (uint32_t)n_mblk);
    const int64_t pt0 = (int64_t)(unit / (uint32_t)n_mblk) * (32 * TR_T);
    if (pt0 >= M) return;
    const int mt0 = mblk * TR_MTB;
    const int KT = c_in / 32;
    int64_t prow[TR_T];
#pragma unroll
    for (int j = 0; j < TR_T; ++j) prow[j] = min(pt0 + 32 * j, M - 32) + m;
    WRing<DAL3_PF> ring;
    ring.init(wpk + (int64_t)mblk * KT * 16 * 64, lane);
    f32x16 acc[TR_T][TR_MTB];
#pragma unroll
    for (int t = 0; t < TR_MTB; ++t) {
        const float bv = bias ? bias[32 * (mt0 + t) + m] : 0.0f;     // this lane's CHANNEL; the same for all 16 point rows
#pragma unroll
        for (int j = 0; j < TR_T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][t][r] = bv;
    }
    TrX<TR_T> xa, xb;
    tr_load_x(xa, 0, a, lda, prow, h);
    for (int kt = 0; kt < KT; kt += 2) {
        tr_load_x(xb, min(kt + 1, KT - 1), a, lda, prow, h);
        DAL3_SCHED_FENCE();
        if (act) tr_act_lds(xa.X, s_sc, s_sh, kt, h, relu_in);
        tr_ring_block<TR_T, TR_MTB, 0, true>(ring, xa.X, acc);
        tr_load_x(xa, min(kt + 2, KT - 1), a, lda, prow, h);
        DAL3_SCHED_FENCE();
        if (kt + 1 < KT) {
            if (act) tr_act_lds(xb.X, s_sc, s_sh, kt + 1, h, relu_in);
            tr_ring_block<TR_T, TR_MTB, 0, true>(ring, xb.X, acc);
        }
    }
#pragma unroll
    for (int t = 0; t < TR_MTB; ++t) {
        const int c = 32 * (mt0 + t) + m;
        const float sc = out_scale[c], sh = out_shift[c];
#pragma unroll
        for (int j = 0; j < TR_T; ++j) {
            if (pt0 + 32 * j >= M) break;
            pool_candidate(acc[j][t], sc, sh, h, pt0 + 32 * j, seg, c_out, c, packed);
        }
    }
}

// tr_linear_pool_kernel with persistent waves, as tr_linear_pers_kernel: the next unit's first k-tile is fetched under
// this unit's last MFMAs (a wave of the kernel above waits out one HBM round trip per unit with its matrix pipe idle:
// 13 % of the 128 -> 1024 layer by ablation), the weight ring runs on cyclically, and an output tile's epilogue —
// BN, ReLU, the max over its 32 points, the packed atomicMax — is placed behind the tile's last MFMA, under the MFMAs
// of the tiles that follow. Same FMA chains, same candidates: g and arg are bit-identical to the kernel above.
// Host-side conditions: M % (32 TR_T) == 0, c_in % 64 == 0, n_waves % n_mblk == 0, at least two units per wave.
template <int OCC, int KTC>
__global__ __launch_bounds__(256, OCC) void tr_linear_pool_pers_kernel(const float* __restrict__ a, int64_t M, int c_in, int64_t lda,
                                                                     const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, int relu_in,
                                                                     const f32x4* __restrict__ wpk, const float* __restrict__ bias,
                                                                     const float* __restrict__ out_scale,
                                                                     const float* __restrict__ out_shift, int64_t seg, int c_out,
                                                                     unsigned long long* __restrict__ packed, int n_mblk,
                                                                     uint32_t n_units) {
    __shared__ float s_sc[TR_MAX_ACT_CIN], s_sh[TR_MAX_ACT_CIN];
    const bool act = tr_stage_act(scale, shift, c_in, s_sc, s_sh);
    const int lane = threadIdx.x & 63, h = lane >> 5, m = lane & 31;
    uint32_t unit = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * 4u;
    if (unit >= n_units) return;
    const int mblk = (int)(unit % (uint32_t)n_mblk);
    const int mt0 = mblk * TR_MTB;
    const int KT = KTC ? KTC : c_in / 32;
    WRing<DAL3_PF, true> ring;
    ring.init(wpk + (int64_t)mblk * KT * 16 * 64, lane, (uint32_t)(KT * 16) * 1024u);
    float bch[TR_MTB], osc[TR_MTB], osh[TR_MTB];               // this lane's channel of each output tile
#pragma unroll
    for (int t = 0; t < TR_MTB; ++t) {
        const int c = 32 * (mt0 + t) + m;
        bch[t] = bias ? bias[c] : 0.0f;
        osc[t] = out_scale[c];
        osh[t] = out_shift[c];
    }
    int64_t pt0 = (int64_t)(unit / (uint32_t)n_mblk) * (32 * TR_T);
    int64_t prow[TR_T];
#pragma unroll
    for (int j = 0; j < TR_T; ++j) prow[j] = pt0 + 32 * j + m;
    TrX<TR_T> xa, xb;
    tr_load_x(xa, 0, a, lda, prow, h);
    __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0): see tr_linear_pers_kernel
    for (;;) {
        f32x16 acc[TR_T][TR_MTB];
#pragma unroll
        for (int t = 0; t < TR_MTB; ++t)
#pragma unroll
            for (int j = 0; j < TR_T; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][t][r] = bch[t];
        const uint32_t unit_n = unit + n_waves;
        const bool more = unit_n < n_units;
        const int64_t pt0_n = more ? (int64_t)(unit_n / (uint32_t)n_mblk) * (32 * TR_T) : pt0;
        int64_t prow_n[TR_T];
#pragma unroll
        for (int j = 0; j < TR_T; ++j) prow_n[j] = pt0_n + 32 * j + m;
        auto finish_tile = [&](int t) {                         // the epilogue of tr_linear_pool_kernel for output tile t
#pragma unroll
            for (int j = 0; j < TR_T; ++j)
                pool_candidate(acc[j][t], osc[t], osh[t], h, pt0 + 32 * j, seg, c_out, 32 * (mt0 + t) + m, packed);
        };
        auto kstep = [&](int kt, auto last_c) {
            constexpr bool LAST = decltype(last_c)::value;
            tr_load_x(xb, kt + 1, a, lda, prow, h);
            DAL3_SCHED_FENCE();
            if (act) tr_act_lds(xa.X, s_sc, s_sh, kt, h, relu_in);
            tr_ring_block<TR_T, TR_MTB, 0, true>(ring, xa.X, acc);
            tr_load_x(xa, LAST ? 0 : kt + 2, a, lda, LAST ? prow_n : prow, h);
            DAL3_SCHED_FENCE();
            if (act) tr_act_lds(xb.X, s_sc, s_sh, kt + 1, h, relu_in);
            if (LAST)                                           // an output tile's epilogue behind its last MFMA
                tr_ring_block<TR_T, TR_MTB, 0, true>(ring, xb.X, acc, [&](int i) {
                    if (i % 4 == 3) finish_tile(i / 4);
                });
            else
                tr_ring_block<TR_T, TR_MTB, 0, true>(ring, xb.X, acc);
        };
        if constexpr (KTC == 2) {
            kstep(0, std::true_type{});
        } else {                                               // KT >= 4
            kstep(0, std::false_type{});
            for (int kt = 2; kt + 2 < KT; kt += 2) kstep(kt, std::false_type{});
            kstep(KT - 2, std::true_type{});
        }
        if (!more) break;
        unit = unit_n;
        pt0 = pt0_n;
#pragma unroll
        for (int j = 0; j < TR_T; ++j) prow[j] = prow_n[j];
    }
}

// The 128-channel case (ins_seg's conv5, 128 -> 1024) with the wave's activations RESIDENT: the kernel above loads and
// activates a unit's 64 x 128 inputs once per block of 128 output channels, eight times per point at c_out = 1024 (by
// ablation at 64 x 4096 points: input loads 48 us, activation 71 us, epilogue 95 us of 627; the MFMAs alone 459). Here a
// wave takes 64 points, loads and activates them ONCE (128 registers), and sweeps all output tiles over them, the
// weights arriving in tile-major order (tr_pack_kernel with mtb = 1) through the same cyclic ring: one turn of the
// stream per group of points.
//  * Two accumulator sets alternate, and the epilogue of the tile just finished — BN, ReLU, running (max, index) over its
//    16 registers — is dealt out one register per weight fragment under the MFMAs of the tile being computed.
//  * A wave's groups are CONSECUTIVE (gpw of them, all in one segment when seg % (64 gpw) == 0), and its candidates meet
//    in a private LDS row per output channel (ds_max_u64, counted by lgkmcnt); the packed global atomicMax — which sits
//    in the same in-order vmcnt queue as the weight ring's loads — is taken once per wave and segment, not per tile.
//  * The next group's 64 x 128 inputs are requested under the second tile of the current one (two loads per fragment),
//    so the switch costs the activation's VALU only (by ablation the simultaneous reload of all waves was ~40 us).
// Same FMA chains per output element, same candidate order: g and arg are bit-identical to the kernels above.
// Host-side conditions: c_in == 128, M % 64 == 0, seg % 64 == 0, c_out % 64 == 0, c_out <= TR_POOL_RES_MAX_COUT.
#define TR_POOL_RES_MAX_COUT 1024
__global__ __launch_bounds__(256, 1) void tr_linear_pool_res_kernel(const float* __restrict__ a, int64_t M, int64_t lda,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, int relu_in,
                                                                  const f32x4* __restrict__ wpk, const float* __restrict__ bias,
                                                                  const float* __restrict__ out_scale,
                                                                  const float* __restrict__ out_shift, int64_t seg, int c_out,
                                                                  unsigned long long* __restrict__ packed, uint32_t n_groups,
                                                                  uint32_t gpw) {
    __shared__ float s_sc[128], s_sh[128];
    __shared__ float s_b[TR_POOL_RES_MAX_COUT], s_osc[TR_POOL_RES_MAX_COUT], s_osh[TR_POOL_RES_MAX_COUT];
    __shared__ unsigned long long s_key[4][TR_POOL_RES_MAX_COUT];
    const bool act = scale != nullptr;
    for (int i = threadIdx.x; i < 128; i += 256) {
        s_sc[i] = act ? scale[i] : 1.0f;
        s_sh[i] = act ? shift[i] : 0.0f;
    }
    for (int i = threadIdx.x; i < c_out; i += 256) {
        s_b[i] = bias ? bias[i] : 0.0f;
        s_osc[i] = out_scale[i];
        s_osh[i] = out_shift[i];
    }
    for (int i = threadIdx.x; i < 4 * TR_POOL_RES_MAX_COUT; i += 256) (&s_key[0][0])[i] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, m = lane & 31;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long* key = s_key[wv];
    uint32_t group = (blockIdx.x * 4u + wv) * gpw;
    if (group >= n_groups) return;
    const uint32_t group_end = min(group + gpw, n_groups);
    WRing<DAL3_PF, true> ring;
    ring.init(wpk, lane, (uint32_t)c_out * 128u * 4u);
    const int n_tiles = c_out / 32;
    auto flush = [&](int64_t s_idx) {                           // this wave's candidates of segment s_idx -> packed, row cleared
        for (int c = lane; c < c_out; c += 64) {
            const unsigned long long k = key[c];
            if (k) atomicMax(packed + s_idx * c_out + c, k);
            key[c] = 0ull;
        }
    };
    TrX<2> x[4], xn[4];
    {
        const int64_t prow[2] = {(int64_t)group * 64 + m, (int64_t)group * 64 + 32 + m};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) tr_load_x(xn[kt], kt, a, lda, prow, h);
    }
    int64_t cur_seg = (int64_t)((uint32_t)((int64_t)group * 64) / (uint32_t)seg);
    for (; group < group_end; ++group) {
        const int64_t pt0 = (int64_t)group * 64;
        const int64_t s_idx = (int64_t)((uint32_t)pt0 / (uint32_t)seg);
        if (s_idx != cur_seg) {
            flush(cur_seg);
            cur_seg = s_idx;
        }
        const uint32_t in_seg0 = (uint32_t)(pt0 - s_idx * seg);
        // the group's inputs arrived under the previous group's second tile: activation, and the registers change roles
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            x[kt] = xn[kt];
            if (act) tr_act_lds(x[kt].X, s_sc, s_sh, kt, h, relu_in);
        }
        const bool more = group + 1 < group_end;
        const int64_t pn = more ? pt0 + 64 : pt0;
        const int64_t prow_n[2] = {pn + m, pn + 32 + m};
        f32x16 accA[2], accB[2];
        float bv[2] = {0.0f, 0.0f};
        int bi[2] = {4 * h, 4 * h};                             // (this lane's first point: what a tile of zeros returns)
        // per-lane constants of the tiles, read from LDS half a tile ahead: bias of the NEXT tile, BN affine of THIS one
        // (needed when it is the pending one)
        float b_nx = s_b[m], osc_nx = 0.0f, osh_nx = 0.0f, posc = 0.0f, posh = 0.0f;
        // one register (both point tiles) of the pending tile's epilogue. The empty asm pins each step where it is written:
        // left alone hipcc sinks one point tile's whole chain (16 x fma, max, cmp, 2 cndmask with their VCC wait states)
        // behind the tile's last MFMA, ~1,000 cycles per tile with the matrix pipe idle
        auto epi_step = [&](const f32x16 (&P)[2], int r) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // (the ReLU is taken once, on the running maximum, in epi_finish: max and ReLU commute, and the first index
                // attaining a positive maximum is the same before and after it; a maximum <= 0 means every value is 0
                // after the ReLU, whose first maximum is index 0 — the initial bi, kept because bv starts at 0)
                const float y = __builtin_fmaf(P[j][r], posc, posh);
                const bool up = y > bv[j];
                bv[j] = up ? y : bv[j];
                bi[j] = up ? (r & 3) + 8 * (r >> 2) + 4 * h : bi[j];
            }
            asm volatile("" : "+v"(bv[0]), "+v"(bv[1]), "+v"(bi[0]), "+v"(bi[1]));
        };
        // the pending tile's candidates leave: as keys (pool_key: the larger key is the larger value, at equal values
        // the earlier point) the two point tiles and the two lane halves meet by plain 64-bit maxima; the
        // halves are exchanged by v_permlane32_swap (no LDS round trip), the lower half's lanes write
        auto epi_finish = [&](int ptile) {
            uint32_t kh = 0, kl = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned long long k = pool_key(bv[j], in_seg0 + 32u * j + (uint32_t)bi[j]);
                const uint32_t vh = (uint32_t)(k >> 32), vl = (uint32_t)k;      // (the key's words travel separately: 32-bit compares and swaps)
                const bool up = j == 0 || vh > kh || (vh == kh && vl > kl);
                kh = up ? vh : kh;
                kl = up ? vl : kl;
                bv[j] = 0.0f;
                bi[j] = 4 * h;
            }
            const uint32_t oh = __builtin_amdgcn_permlane32_swap(kh, kh, false, false)[1];
            const uint32_t ol = __builtin_amdgcn_permlane32_swap(kl, kl, false, false)[1];
            const unsigned long long k0 = ((unsigned long long)kh << 32) | kl, k1 = ((unsigned long long)oh << 32) | ol;
            if (h == 0) atomicMax(key + 32 * ptile + m, k0 > k1 ? k0 : k1);
        };
        // tile `t` into Cc while the epilogue of tile t - 1 (in P) runs; pending: there is one; pf: request the next group
        auto tile = [&](f32x16 (&Cc)[2], const f32x16 (&P)[2], int t, auto pending_c, auto pf_c) {
            constexpr bool pending = decltype(pending_c)::value, pf = decltype(pf_c)::value;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) Cc[j][r] = b_nx;
            posc = osc_nx;
            posh = osh_nx;
#pragma unroll
            for (int i = 0; i < 16; ++i) {                      // fragment (kt, q) = (i / 4, i % 4)
                const f32x4 w = ring.slot[i % DAL3_PF];
                ring.slot[i % DAL3_PF] = ring.fetch();
                if (pf) {                                       // two of the next group's 32 16-byte pieces per fragment
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int id = 2 * i + u, kt = id >> 3, j = (id >> 2) & 1, q = id & 3;
                        const f32x4 v = *reinterpret_cast<const f32x4*>(a + prow_n[j] * lda + 32 * kt + 4 * h + 8 * q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) xn[kt].X[j][4 * q + e] = v[e];
                    }
                }
                if (i == 8) {
                    b_nx = s_b[(32 * (t + 1) + m) & (TR_POOL_RES_MAX_COUT - 1)];
                    osc_nx = s_osc[32 * t + m];
                    osh_nx = s_osh[32 * t + m];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) Cc[j] = mfma32(x[i / 4].X[j][4 * (i % 4) + e], w[e], Cc[j]);
                }
                if (pending) {
                    epi_step(P, i);
                    if (i == 15) epi_finish(t - 1);
                }
                DAL3_SCHED_FENCE();
            }
        };
        tile(accA, accB, 0, std::false_type{}, std::false_type{});
        tile(accB, accA, 1, std::true_type{}, std::true_type{});
        for (int t = 2; t < n_tiles; t += 2) {
            tile(accA, accB, t, std::true_type{}, std::false_type{});
            tile(accB, accA, t + 1, std::true_type{}, std::false_type{});
        }
        posc = osc_nx;
        posh = osh_nx;
#pragma unroll
        for (int r = 0; r < 16; ++r) epi_step(accB, r);
        epi_finish(n_tiles - 1);
    }
    flush(cur_seg);
}

#ifndef TR_POOL_OCC
#define TR_POOL_OCC 1                   // (at 2 the persistent kernel spills 120-170 registers)
#endif
hipError_t launch_tr_linear_pool(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                 int relu_in, const float* W, int64_t ldw, const float* bias, const float* out_scale,
                                 const float* out_shift, int64_t seg, int c_out, float* g, int32_t* arg, float* ws,
                                 unsigned long long* packed, hipStream_t s) {
    const int n_mblk = c_out / 128;
    const int64_t units = ((M + 32 * TR_T - 1) / (32 * TR_T)) * n_mblk;
    const int64_t n_seg = M / seg;
    hipError_t e = launch_fill_words(packed, (size_t)n_seg * c_out * 2, 0u, s);
    if (e != hipSuccess) return e;
    const auto wpk = reinterpret_cast<const f32x4*>(ws);
    const unsigned pers_grid = 256u * TR_POOL_OCC;
    // (the 128-channel case through the per-block kernels instead: profiles/LEDGER_r04.md 2.1 item 9)
    if (c_in == 128 && M % 64 == 0 && seg % 64 == 0 && c_out % 64 == 0 && c_out <= TR_POOL_RES_MAX_COUT && M / 64 >= 1024 &&
        M < (int64_t)1 << 31) {                             // (point indices are taken as 32-bit values inside)
        const uint32_t n_groups = (uint32_t)(M / 64), gpw = (n_groups + 1023u) / 1024u;
        tr_pack(W, ldw, 0, c_out, c_in, 1, ws, s);
        hipLaunchKernelGGL(tr_linear_pool_res_kernel, dim3((n_groups + 4u * gpw - 1u) / (4u * gpw)), dim3(256), 0, s, a, M, lda, scale, shift,
                           relu_in, wpk, bias, out_scale, out_shift, seg, c_out, packed, n_groups, gpw);
    } else {
        tr_pack(W, ldw, 0, c_out, c_in, TR_MTB, ws, s);
        const auto pers = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(pers_grid), dim3(256), 0, s, a, M, c_in, lda, scale, shift, relu_in, wpk, bias, out_scale,
                               out_shift, seg, c_out, packed, n_mblk, (uint32_t)units);
        };
        if (M % (32 * TR_T) != 0 || c_in % 64 != 0 || (4 * pers_grid) % (unsigned)n_mblk != 0 || units < 2 * 4 * (int64_t)pers_grid ||
            units >= (int64_t)1 << 31)
            hipLaunchKernelGGL(tr_linear_pool_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a, M, c_in, lda, scale, shift,
                               relu_in, wpk, bias, out_scale, out_shift, seg, c_out, packed, n_mblk);
        else if (c_in == 64)
            pers(tr_linear_pool_pers_kernel<TR_POOL_OCC, 2>);
        else
            pers(tr_linear_pool_pers_kernel<TR_POOL_OCC, 0>);
    }
    return launch_tr_segmax_unpack(packed, n_seg * c_out, g, arg, s);
}

// every layer with whole 32-channel tiles can take a ring path (which one depends on M: see launch_tr_linear)
size_t tr_linear_workspace_bytes(int c_in, int c_out) {
    return c_out % 32 == 0 ? (size_t)c_out * c_in * sizeof(float) + DAL3_PF * 1024 : 0;
}

#define TR_SMALL_M 256                   // at most this many rows: one 32 x 32 output tile per wave (<1, 1>)

template <int T, int MTB, int OCC>
static bool tr_linear_pers_ok(int64_t M, int c_in, int64_t seg, int c_out, int accumulate) {
    const int n_mblk = c_out / (32 * MTB);
    const int64_t units = ((M + 32 * T - 1) / (32 * T)) * n_mblk;
    const unsigned pers_grid = 256u * OCC;                  // one workgroup per wave slot: 4 * pers_grid waves
    return MTB >= 2 && c_out % (32 * MTB) == 0 && !accumulate && M % (32 * T) == 0 &&
           (seg == 0 || seg % (32 * T) == 0) && c_in % 64 == 0 && (4 * pers_grid) % (unsigned)n_mblk == 0 &&
           units >= 2 * 4 * (int64_t)pers_grid && units < (int64_t)1 << 31;
}

template <int T, int MTB, int OCC>
struct TrTile {};                                           // names an instantiation of the ring kernels (deduced by the launcher below)
template <int T, int MTB, int OCC>
static void tr_linear_ring_launch(TrTile<T, MTB, OCC>, const float* a, int64_t M, int c_in, int64_t lda, const float* scale,
                                  const float* shift, int relu_in, const float* W, int64_t ldw, int transpose_w, const float* bias,
                                  int64_t seg, int c_out, float* z, int64_t ldz, int accumulate, float* ws, hipStream_t s,
                                  bool prepacked, int red_mode = 0, const TrRed* red = nullptr) {
    const int n_mblk = c_out / (32 * MTB);
    const int64_t units = ((M + 32 * T - 1) / (32 * T)) * n_mblk;
    if (!prepacked) tr_pack(W, ldw, transpose_w, c_out, c_in, MTB, ws, s);   // (prepacked: ws already holds this layer in fragment order, MTB = this path's)
    const int KT = c_in / 32;
    const unsigned pers_grid = 256u * OCC;
    if constexpr (MTB >= 2) {
        // (the persistent kernel's transposed stores address a unit's 64 rows with 32-bit byte offsets: row strides beyond
        // 2^22 floats — no tensor of this path comes near — take the one-unit-per-wave kernel)
        if (tr_linear_pers_ok<T, MTB, OCC>(M, c_in, seg, c_out, accumulate) && ldz < ((int64_t)1 << 22)) {
            const TrRed rd = red ? *red : TrRed{};
            const auto args = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(pers_grid), dim3(256), 0, s, a, M, c_in, lda, scale, shift, relu_in,
                                   reinterpret_cast<const f32x4*>(ws), bias, seg, c_out, z, ldz, n_mblk, (uint32_t)units, rd);
            };
            const auto pick = [&](auto red_c) {
                constexpr int RED = decltype(red_c)::value;
                if (KT == 2) {
                    args(tr_linear_pers_kernel<T, MTB, OCC, 2, RED>);
                } else if (KT == 4 && MTB == 4) {              // (<2, 2, 2, 4> spills 64 registers; the generic one does not)
                    if constexpr (MTB == 4) args(tr_linear_pers_kernel<T, MTB, OCC, 4, RED>);
                } else {
                    args(tr_linear_pers_kernel<T, MTB, OCC, 0, RED>);
                }
            };
            if constexpr (MTB == 4) {
                if (red_mode == 1)
                    pick(std::integral_constant<int, 1>{});
                else if (red_mode == 2)
                    pick(std::integral_constant<int, 2>{});
                else
                    pick(std::integral_constant<int, 0>{});
            } else {                                           // (tr_linear_red_ok: forward statistics of K = 64 only)
                if (red_mode == 1 && KT == 2)
                    args(tr_linear_pers_kernel<T, MTB, OCC, 2, 1>);
                else
                    pick(std::integral_constant<int, 0>{});
            }
            return;
        }
    }
    hipLaunchKernelGGL((tr_linear_ring_kernel<T, MTB, OCC>), dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a, M, c_in, lda,
                       scale, shift, relu_in, reinterpret_cast<const f32x4*>(ws), bias, seg, c_out, z, ldz, accumulate,
                       n_mblk);
}

// Which kernel family a layer takes — the ONE place that decides it (launch_tr_linear and the pack plan both ask):
// 0: the strided-weight kernel (no packed weights); otherwise the ring path's output tiles per wave (1, 2 or TR_MTB),
// with *small set when M <= TR_SMALL_M (the <1, 1, 2> instantiation).
// K <= 128 through the one-unit-per-wave kernel: a wave's whole K loop is a few microseconds, about as long as its
// prologue and its stores; the smaller <2, 2> tile fits two waves per SIMD, so one wave's ends run under the other's
// MFMAs (64 -> 512: 282 -> 258 us). Where the persistent kernel applies it overlaps the ends itself and the big tile
// wins again (64 -> 512: 185 us)
#ifndef TR_SMALL_K
#define TR_SMALL_K 128
#endif
static int tr_linear_path(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, bool has_ws, bool has_act, bool* small) {
    const bool ring_ok = has_ws && c_out % 32 == 0 && (!has_act || c_in <= TR_MAX_ACT_CIN);
    *small = false;
    if (!ring_ok) return 0;
    if (M <= TR_SMALL_M) {
        *small = true;
        return 1;
    }
    if (c_out % 128 == 0 && (c_in > TR_SMALL_K || tr_linear_pers_ok<TR_T, TR_MTB, TR_RING_OCC>(M, c_in, seg, c_out, accumulate)))
        return TR_MTB;
    if (c_out % 64 == 0) return 2;
    return 1;
}
int tr_linear_pack_mtb(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, int has_act) {
    bool small;
    return tr_linear_path(M, c_in, seg, c_out, accumulate, true, has_act != 0, &small);
}

hipError_t launch_tr_pack_many(const dal3_tr_pack_item* items, int n, hipStream_t s) {
    if (n <= 0 || n > TR_PACK_MAX) return hipErrorInvalidValue;
    TrPackMany p;
    p.n = n;
    uint32_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const dal3_tr_pack_item& t = items[i];
        p.it[i] = TrPackItem{t.W, t.out, t.ldw, t.transpose_w, t.c_out, t.c_in, t.mtb, blocks};
        blocks += (uint32_t)(((int64_t)t.c_out * t.c_in * ((t.mtb & 0x100) ? 2 : 1) + 255) / 256);
    }
    hipLaunchKernelGGL(tr_pack_many_kernel, dim3(blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tr_linear(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                            int relu_in, const float* W, int64_t ldw, int transpose_w, const float* bias, int64_t seg,
                            int c_out, float* z, int64_t ldz, int accumulate, float* ws, hipStream_t s, bool prepacked) {
    bool small;
    const int mtb = tr_linear_path(M, c_in, seg, c_out, accumulate, ws != nullptr, scale != nullptr, &small);
    const auto ring = [&](auto tile) {
        tr_linear_ring_launch(tile, a, M, c_in, lda, scale, shift, relu_in, W, ldw, transpose_w, bias, seg, c_out, z, ldz, accumulate,
                              ws, s, prepacked);
    };
    if (small) {
        ring(TrTile<1, 1, 2>{});
    } else if (mtb == TR_MTB) {
        ring(TrTile<TR_T, TR_MTB, TR_RING_OCC>{});
    } else if (mtb == 2) {
        ring(TrTile<TR_T, 2, 2>{});
    } else if (mtb == 1) {                                  // c_out = 32, 96, ...: one output tile per wave
        ring(TrTile<TR_T, 1, 2>{});
    } else {
        const int n_mblk = (c_out / 32 + TR_MTB - 1) / TR_MTB;
        const int64_t units = ((M + 32 * TR_T - 1) / (32 * TR_T)) * n_mblk;
        hipLaunchKernelGGL(tr_linear_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, a, M, c_in, lda, scale, shift,
                           relu_in, W, ldw, transpose_w, bias, seg, c_out, z, ldz, accumulate, n_mblk);
    }
    return hipGetLastError();
}

// A linear layer whose epilogue takes a column reduction of its output (TrRed; tr_linear_pers_kernel RED): the shapes
// the persistent kernels take, with room for the transposed tile's 32-bit lane offsets. *n_part = partial rows written
// per channel (one per wave of a channel block) = what the second stage (tr_colred_final_kernel) must be told.
bool tr_linear_red_ok(int red_mode, int64_t M, int c_in, int64_t seg, int c_out, bool has_ws, bool has_act, int64_t ldz, int64_t ldbz,
                      int* n_part) {
    bool small;
    const int mtb = tr_linear_path(M, c_in, seg, c_out, 0, has_ws, has_act, &small);
    if (small || ldz >= ((int64_t)1 << 22) || ldbz >= ((int64_t)1 << 22)) return false;     // (64 rows x ld x 4 B < 2^31)
    if (mtb == TR_MTB && tr_linear_pers_ok<TR_T, TR_MTB, TR_RING_OCC>(M, c_in, seg, c_out, 0)) {
        *n_part = (int)(4u * 256u * TR_RING_OCC) / (c_out / (32 * TR_MTB));
        return true;
    }
    // the two-output-tile kernel runs two waves per SIMD (256 registers): only the forward statistics of a K = 64 layer
    // fit without spilling (conv2 / conv3 of ins_seg); the other combinations keep the separate pass
    if (mtb == 2 && red_mode == 1 && c_in == 64 && tr_linear_pers_ok<TR_T, 2, 2>(M, c_in, seg, c_out, 0)) {
        *n_part = (int)(4u * 256u * 2) / (c_out / 64);
        return true;
    }
    return false;
}
// (n_part * c_out is 4 * 256 * OCC * 32 * MTB channels-rows whatever the layer: 2 MiB of float64 pairs at most)
size_t tr_linear_red_workspace_bytes() { return (size_t)2048 * 128 * 2 * sizeof(double); }

// precondition: tr_linear_red_ok(...) and a packed weight image in ws
static hipError_t launch_tr_linear_red(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                       int relu_in, const float* W, int64_t ldw, int transpose_w, const float* bias, int64_t seg,
                                       int c_out, float* z, int64_t ldz, float* ws, hipStream_t s, int red_mode, const TrRed& red) {
    bool small;
    const int mtb = tr_linear_path(M, c_in, seg, c_out, 0, true, scale != nullptr, &small);
    const auto ring = [&](auto tile) {
        tr_linear_ring_launch(tile, a, M, c_in, lda, scale, shift, relu_in, W, ldw, transpose_w, bias, seg, c_out, z, ldz, 0, ws, s,
                              true, red_mode, &red);
    };
    if (mtb == TR_MTB)
        ring(TrTile<TR_T, TR_MTB, TR_RING_OCC>{});
    else
        ring(TrTile<TR_T, 2, 2>{});
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- column sums
// Two-stage, fixed-order reductions over the points (deterministic): stage 1 writes one double partial per
// (row block, channel), stage 2 adds the partials of a channel in index order.
// mode 0: s0 = sum z, s1 = sum z^2                                   (batch statistics)
// mode 1: dy = da * [z*scale+shift > 0];  s0 = sum dy (= dbeta), s1 = sum dy * xhat (= dgamma), xhat = (z - mu)*rstd
// da may be NULL with (dg, arg): da[p][c] = (p == arg[seg_of_p][c]) ? dg[seg_of_p][c] : 0   (the max over points)
#define TR_RED_ROWS 256
struct DaSrc {
    const float* da;       // dense (M x C) or NULL
    int64_t ldda;
    const float* dg;       // (M/seg x C) when da == NULL
    const int32_t* arg;    // (M/seg x C) point index within the segment
    int64_t seg;
    __device__ __forceinline__ float at(int64_t p, int c, int C) const {
        if (da) return da[p * ldda + c];
        const int64_t s = p / seg;
        return arg[s * C + c] == (int32_t)(p - s * seg) ? dg[s * C + c] : 0.0f;
    }
};

template <int MODE, bool DENSE>
__global__ __launch_bounds__(256) void tr_colred_kernel(const float* __restrict__ z, int64_t M, int C, int64_t ldz,
                                                        DaSrc src, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ mu,
                                                        const float* __restrict__ rstd, double* __restrict__ part,
                                                        float* __restrict__ act_out = nullptr, int64_t ldo = 0, int relu = 0) {
    // block: 16 groups of 4 channels (float4 loads: a 256-B row segment per 16 lanes) x 16 row-lanes;
    // rows [blockIdx.y*TR_RED_ROWS, +TR_RED_ROWS); C % 4 == 0 (channels are padded to 32)
    __shared__ double sm[2][16][64];
    const int gl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = (blockIdx.x * 16 + gl) * 4;
    const int64_t r0 = (int64_t)blockIdx.y * TR_RED_ROWS;
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    if (c < C) {
        constexpr int mode = MODE;                         // (compile time: a run-time mode is a branch per element to hipcc)
        f32x4 sc = {0, 0, 0, 0}, sh = sc, mean = sc, rs = sc;
        if (mode == 1) {
            sc = *reinterpret_cast<const f32x4*>(scale + c);
            sh = *reinterpret_cast<const f32x4*>(shift + c);
            mean = *reinterpret_cast<const f32x4*>(mu + c);
            rs = *reinterpret_cast<const f32x4*>(rstd + c);
        }
        if (mode == 2) {                                   // (mode 2: y = act(z) written to act_out, s0 = sum y, s1 = sum y^2)
            sc = f32x4{1, 1, 1, 1};
            if (scale) {
                sc = *reinterpret_cast<const f32x4*>(scale + c);
                sh = *reinterpret_cast<const f32x4*>(shift + c);
            }
        }
        const int64_t r1 = min(M, r0 + TR_RED_ROWS);
        // eight rows per trip, their loads issued together (a trip is one HBM round trip: with one row per trip the
        // 64-channel layers ran at 2 TB/s); rows past the end are clamped and masked, the order of the adds is unchanged
        constexpr int U = 8;
        for (int64_t p0 = r0 + rl; p0 < r1; p0 += 16 * U) {
            f32x4 v4[U], d4[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t p = min(p0 + 16 * u, M - 1);
                v4[u] = *reinterpret_cast<const f32x4*>(z + p * ldz + c);
                if (mode == 1) {
                    if (DENSE) {
                        d4[u] = *reinterpret_cast<const f32x4*>(src.da + p * src.ldda + c);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) d4[u][e] = src.at(p, c + e, C);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (p0 + 16 * u >= r1) break;
                const f32x4 v = v4[u];
                if (mode == 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s0[e] += v[e];
                        s1[e] += (double)v[e] * v[e];
                    }
                } else if (mode == 2) {
                    f32x4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float t = __builtin_fmaf(v[e], sc[e], sh[e]);
                        y[e] = relu ? fmaxf(t, 0.0f) : t;
                        s0[e] += y[e];
                        s1[e] += (double)y[e] * y[e];
                    }
                    *reinterpret_cast<f32x4*>(act_out + (p0 + 16 * u) * ldo + c) = y;
                } else {
                    const f32x4 d = d4[u];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float y = v[e] * sc[e] + sh[e];
                        const float dy = y > 0.0f ? d[e] : 0.0f;
                        s0[e] += dy;
                        s1[e] += (double)dy * ((v[e] - mean[e]) * rs[e]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sm[0][rl][gl * 4 + e] = s0[e];
        sm[1][rl][gl * 4 + e] = s1[e];
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cc = blockIdx.x * 64 + threadIdx.x;
        if (cc < C) {
            double t0 = 0.0, t1 = 0.0;
            for (int i = 0; i < 16; ++i) {
                t0 += sm[0][i][threadIdx.x];
                t1 += sm[1][i][threadIdx.x];
            }
            const int64_t o = ((int64_t)blockIdx.y * C + cc) * 2;
            part[o] = t0;
            part[o + 1] = t1;
        }
    }
}

// TR_FIN_CH channels x TR_FIN_L partial-lanes per block: lane l adds the partials l, l + L, l + 2 L, ... (in four interleaved chains),
// then the L lane sums are added in lane order — a fixed association, so the result is reproducible. What follows the sums is
// folded in (EPI): nothing (0: the sums themselves), the forward BatchNorm epilogue (1: batch mean / biased variance ->
// mu, rstd, the folded affine scale = gamma*rstd, shift = beta - mean*scale, and the running statistics' update with
// momentum and unbiased variance exactly as torch's BatchNorm1d does it), or the backward one (2: dbeta = sum dy,
// dgamma = sum dy*xhat, and the coefficients of dz = k1*(dy - k2 - xhat*k3)) — a layer's statistics are two launches,
// not three (the third was 15 us of launch latency for a few hundred bytes, 22 times per training step).
struct BnEpi {
    int64_t M;
    const float* gamma;
    const float* beta;          // forward
    float* running_mean;
    float* running_var;
    float momentum, eps;
    float* mu;                  // forward: out
    float* rstd;                // forward: out; backward: in
    float* scale;               // forward: out
    float* shift;
    float* dgamma;              // backward: out
    float* dbeta;
    float* k1;
    float* k2;
    float* k3;
};

#ifndef TR_FIN_CH
#define TR_FIN_CH 4
#endif
#define TR_FIN_L (256 / TR_FIN_CH)
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <int EPI>
__global__ __launch_bounds__(256) void tr_colred_final_kernel(const double* __restrict__ part, int n_blocks, int C,
                                                              double* __restrict__ out, BnEpi e) {
    // TR_FIN_CH channels x TR_FIN_L partial-lanes per block (round 4: 4 x 64, was 16 x 16 — a 64-channel layer was FOUR
    // workgroups each walking 1024–2048 partial rows in 16 dependent trips, ~7 us thirty times a step; now 16 workgroups
    // and 4–8 trips). Lane l adds rows l, l + L, ... in four interleaved chains, the lane sums are added in lane order:
    // a fixed association.
    __shared__ double sm[2][TR_FIN_L][TR_FIN_CH];
    const int cl = threadIdx.x % TR_FIN_CH, l = threadIdx.x / TR_FIN_CH;
    const int c = blockIdx.x * TR_FIN_CH + cl;
    double s0 = 0.0, s1 = 0.0;
    if (c < C) {
        double u0[4] = {0, 0, 0, 0}, u1[4] = {0, 0, 0, 0};
        int b = l;
        for (; b + 3 * TR_FIN_L < n_blocks; b += 4 * TR_FIN_L) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f64x2 v = *reinterpret_cast<const f64x2*>(part + ((int64_t)(b + TR_FIN_L * k) * C + c) * 2);
                u0[k] += v[0];
                u1[k] += v[1];
            }
        }
        for (; b < n_blocks; b += TR_FIN_L) {
            const f64x2 v = *reinterpret_cast<const f64x2*>(part + ((int64_t)b * C + c) * 2);
            u0[0] += v[0];
            u1[0] += v[1];
        }
        s0 = (u0[0] + u0[1]) + (u0[2] + u0[3]);
        s1 = (u1[0] + u1[1]) + (u1[2] + u1[3]);
    }
    sm[0][l][cl] = s0;
    sm[1][l][cl] = s1;
    __syncthreads();
    if (l == 0 && c < C) {
        double t0 = 0.0, t1 = 0.0;
        for (int i = 0; i < TR_FIN_L; ++i) {
            t0 += sm[0][i][cl];
            t1 += sm[1][i][cl];
        }
        if (EPI == 0) {
            out[c] = t0;
            out[C + c] = t1;
        } else if (EPI == 3) {
            // float32 results in the caller's layout (e.mu), e.M the layout code — round 4: the float64 sums of the narrow
            // layers' weight gradients were converted, transposed and sliced by three stock launches per layer
            float* o = e.mu;
            const int mode = (int)(e.M & 0xff), kin = (int)((e.M >> 8) & 0xff), cuse = (int)(e.M >> 16);
            if (mode == 1) {                                // conv1: column c holds entries i = 2c, 2c + 1 of dW[ch][k], i = ch * kin + k
                const int i0 = 2 * c, i1 = 2 * c + 1;
                if (i0 % kin < cuse) o[(i0 / kin) * cuse + i0 % kin] = (float)t0;
                if (i1 % kin < cuse) o[(i1 / kin) * cuse + i1 % kin] = (float)t1;
            } else {                                        // head2: dW[0][c], dW[1][c] for c < 128, then db[0], db[1]
                if (c < 128) {
                    o[c] = (float)t0;
                    o[128 + c] = (float)t1;
                } else {
                    o[256 + (c - 128)] = (float)t0;
                }
            }
        } else if (EPI == 1) {
            const double mean = t0 / (double)e.M;
            double var = t1 / (double)e.M - mean * mean;
            var = var > 0.0 ? var : 0.0;
            const double rs = 1.0 / sqrt(var + (double)e.eps);
            const double sc = (double)e.gamma[c] * rs;
            e.mu[c] = (float)mean;
            e.rstd[c] = (float)rs;
            e.scale[c] = (float)sc;
            e.shift[c] = (float)((double)e.beta[c] - mean * sc);
            if (e.running_mean) {
                e.running_mean[c] = (1.0f - e.momentum) * e.running_mean[c] + e.momentum * (float)mean;
                e.running_var[c] = (1.0f - e.momentum) * e.running_var[c] +
                                   e.momentum * (float)(var * ((double)e.M / (double)(e.M - 1)));
            }
        } else {
            e.dbeta[c] = (float)t0;
            e.dgamma[c] = (float)t1;
            e.k1[c] = e.gamma[c] * e.rstd[c];
            e.k2[c] = (float)(t0 / (double)e.M);
            e.k3[c] = (float)(t1 / (double)e.M);
        }
    }
}

size_t tr_colred_workspace_bytes(int64_t M, int C) {
    return (size_t)((M + TR_RED_ROWS - 1) / TR_RED_ROWS) * C * 2 * sizeof(double);
}

static void colred_partials(const float* z, int64_t M, int C, int64_t ldz, int mode, const DaSrc& src, const float* scale,
                            const float* shift, const float* mu, const float* rstd, double* part, hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    const dim3 grid((C + 63) / 64, nb);
    if (mode == 0)
        hipLaunchKernelGGL((tr_colred_kernel<0, true>), grid, dim3(256), 0, s, z, M, C, ldz, src, scale, shift, mu, rstd, part);
    else if (src.da)
        hipLaunchKernelGGL((tr_colred_kernel<1, true>), grid, dim3(256), 0, s, z, M, C, ldz, src, scale, shift, mu, rstd, part);
    else
        hipLaunchKernelGGL((tr_colred_kernel<1, false>), grid, dim3(256), 0, s, z, M, C, ldz, src, scale, shift, mu, rstd, part);
}

hipError_t launch_tr_colred(const float* z, int64_t M, int C, int64_t ldz, int mode, const float* da, int64_t ldda,
                            const float* dg, const int32_t* arg, int64_t seg, const float* scale, const float* shift,
                            const float* mu, const float* rstd, double* part, double* out, hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    colred_partials(z, M, C, ldz, mode, DaSrc{da, ldda, dg, arg, seg}, scale, shift, mu, rstd, part, s);
    hipLaunchKernelGGL(tr_colred_final_kernel<0>, dim3((C + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, nb, C, out, BnEpi{});
    return hipGetLastError();
}

// out = act(x) AND the float64 column sums of out (sums[0..C) = sum, [C..2C) = sum of squares) in one pass: what the pooled
// layer's moment route needs of its input activation (train.py _moments_through) — was an activation pass + a reduction pass
hipError_t launch_tr_act_colsum(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift, int relu,
                                float* out, int64_t ldo, double* part, double* sums, hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    const dim3 grid((C + 63) / 64, nb);
    hipLaunchKernelGGL((tr_colred_kernel<2, true>), grid, dim3(256), 0, s, x, M, C, ldx, DaSrc{nullptr, 0, nullptr, nullptr, 0}, scale,
                       shift, nullptr, nullptr, part, out, ldo, relu);
    hipLaunchKernelGGL(tr_colred_final_kernel<0>, dim3((C + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, nb, C, sums, BnEpi{});
    return hipGetLastError();
}

// batch statistics of z and everything the forward derives from them (see BnEpi)
hipError_t launch_tr_bn_stats(const float* z, int64_t M, int C, int64_t ldz, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                              float* scale, float* shift, double* part, hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    colred_partials(z, M, C, ldz, 0, DaSrc{nullptr, 0, nullptr, nullptr, 0}, nullptr, nullptr, nullptr, nullptr, part, s);
    BnEpi e{};
    e.M = M, e.gamma = gamma, e.beta = beta, e.running_mean = running_mean, e.running_var = running_var;
    e.momentum = momentum, e.eps = eps, e.mu = mu, e.rstd = rstd, e.scale = scale, e.shift = shift;
    hipLaunchKernelGGL(tr_colred_final_kernel<1>, dim3((C + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, nb, C, nullptr, e);
    return hipGetLastError();
}

// the two sums of the BatchNorm/ReLU backward and its per-channel coefficients
hipError_t launch_tr_bnbwd_sums(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda, const float* dg,
                                const int32_t* arg, int64_t seg, const float* scale, const float* shift, const float* mu,
                                const float* rstd, const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2,
                                float* k3, double* part, hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    colred_partials(z, M, C, ldz, 1, DaSrc{da, ldda, dg, arg, seg}, scale, shift, mu, rstd, part, s);
    BnEpi e{};
    e.M = M, e.gamma = gamma, e.rstd = const_cast<float*>(rstd), e.dgamma = dgamma, e.dbeta = dbeta, e.k1 = k1, e.k2 = k2, e.k3 = k3;
    hipLaunchKernelGGL(tr_colred_final_kernel<2>, dim3((C + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, nb, C, nullptr, e);
    return hipGetLastError();
}

// z = linear(...) and the batch statistics of z (launch_tr_bn_stats of the output) — in the linear kernel's epilogue when
// the shape takes the persistent kernel and every row is real (rows == M: padding rows would enter the sums), else as the
// two separate steps. `part`: max(tr_colred_workspace_bytes(rows, c_out), tr_linear_red_workspace_bytes()).
hipError_t launch_tr_linear_bn_stats(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                     int relu_in, const float* W, int64_t ldw, const float* bias, int64_t seg, int c_out,
                                     float* z, int64_t ldz, float* packed, int64_t rows, const float* gamma, const float* beta,
                                     float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                     float* bn_scale, float* bn_shift, double* part, hipStream_t s, int* fused) {
    int n_part = 0;
    *fused = rows == M && tr_linear_red_ok(1, M, c_in, seg, c_out, true, scale != nullptr, ldz, 0, &n_part);
    if (!*fused) {
        hipError_t e = launch_tr_linear(a, M, c_in, lda, scale, shift, relu_in, W, ldw, 0, bias, seg, c_out, z, ldz, 0, packed, s, true);
        if (e != hipSuccess) return e;
        return launch_tr_bn_stats(z, rows, c_out, ldz, gamma, beta, running_mean, running_var, momentum, eps, mu, rstd, bn_scale,
                                  bn_shift, part, s);
    }
    TrRed red{};
    red.part = part;
    hipError_t e = launch_tr_linear_red(a, M, c_in, lda, scale, shift, relu_in, W, ldw, 0, bias, seg, c_out, z, ldz, packed, s, 1, red);
    if (e != hipSuccess) return e;
    BnEpi ep{};
    ep.M = rows, ep.gamma = gamma, ep.beta = beta, ep.running_mean = running_mean, ep.running_var = running_var;
    ep.momentum = momentum, ep.eps = eps, ep.mu = mu, ep.rstd = rstd, ep.scale = bn_scale, ep.shift = bn_shift;
    hipLaunchKernelGGL(tr_colred_final_kernel<1>, dim3((c_out + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, n_part, c_out, nullptr, ep);
    return hipGetLastError();
}

// da = dz W (a dgrad: transposed weight image) and the BatchNorm-backward sums of the layer that da belongs to
// (launch_tr_bnbwd_sums with da = the output, z = bz), fused the same way; c_out here = that layer's channel count.
hipError_t launch_tr_linear_bnbwd_sums(const float* a, int64_t M, int c_in, int64_t lda, const float* W, int64_t ldw, int c_out,
                                       float* da, int64_t ldda, float* packed, int64_t rows, const float* bz, int64_t ldbz,
                                       const float* bscale, const float* bshift, const float* bmu, const float* brstd,
                                       const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3,
                                       double* part, hipStream_t s, int* fused) {
    int n_part = 0;
    *fused = rows == M && tr_linear_red_ok(2, M, c_in, 0, c_out, true, false, ldda, ldbz, &n_part);
    if (!*fused) {
        hipError_t e = launch_tr_linear(a, M, c_in, lda, nullptr, nullptr, 0, W, ldw, 1, nullptr, 0, c_out, da, ldda, 0, packed, s, true);
        if (e != hipSuccess) return e;
        return launch_tr_bnbwd_sums(bz, rows, c_out, ldbz, da, ldda, nullptr, nullptr, 0, bscale, bshift, bmu, brstd, gamma, dgamma,
                                    dbeta, k1, k2, k3, part, s);
    }
    TrRed red{part, bz, ldbz, bscale, bshift, bmu, brstd};
    hipError_t e = launch_tr_linear_red(a, M, c_in, lda, nullptr, nullptr, 0, W, ldw, 1, nullptr, 0, c_out, da, ldda, packed, s, 2, red);
    if (e != hipSuccess) return e;
    BnEpi ep{};
    ep.M = rows, ep.gamma = gamma, ep.rstd = const_cast<float*>(brstd), ep.dgamma = dgamma, ep.dbeta = dbeta, ep.k1 = k1, ep.k2 = k2, ep.k3 = k3;
    hipLaunchKernelGGL(tr_colred_final_kernel<2>, dim3((c_out + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, n_part, c_out, nullptr, ep);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- per-channel epilogues
// One launch instead of a dozen tiny framework ops per layer (the step is otherwise host-bound at these sizes).
// Forward: batch mean / biased variance from the float64 sums, the folded affine (scale = gamma*rstd, shift = beta -
// mean*scale), and the running statistics' update (momentum, unbiased variance) exactly as torch's BatchNorm1d does.
__global__ void tr_bn_finalize_kernel(const double* __restrict__ sums, int C, int64_t M, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, float* __restrict__ running_mean,
                                      float* __restrict__ running_var, float momentum, float eps, float* __restrict__ mu,
                                      float* __restrict__ rstd, float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double mean = sums[c] / (double)M;
    double var = sums[C + c] / (double)M - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double rs = 1.0 / sqrt(var + (double)eps);
    const double sc = (double)gamma[c] * rs;
    mu[c] = (float)mean;
    rstd[c] = (float)rs;
    scale[c] = (float)sc;
    shift[c] = (float)((double)beta[c] - mean * sc);
    if (running_mean) {
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(var * ((double)M / (double)(M - 1)));
    }
}

// Backward: dbeta = sum dy, dgamma = sum dy*xhat, and the three coefficients of dz = k1*(dy - k2 - xhat*k3).
__global__ void tr_bnbwd_coef_kernel(const double* __restrict__ sums, int C, int64_t M, const float* __restrict__ gamma,
                                     const float* __restrict__ rstd, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                     float* __restrict__ k1, float* __restrict__ k2, float* __restrict__ k3) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    dbeta[c] = (float)sums[c];
    dgamma[c] = (float)sums[C + c];
    k1[c] = gamma[c] * rstd[c];
    k2[c] = (float)(sums[c] / (double)M);
    k3[c] = (float)(sums[C + c] / (double)M);
}

hipError_t launch_tr_bn_finalize(const double* sums, int C, int64_t M, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                 float* scale, float* shift, hipStream_t s) {
    hipLaunchKernelGGL(tr_bn_finalize_kernel, dim3((C + 127) / 128), dim3(128), 0, s, sums, C, M, gamma, beta, running_mean,
                       running_var, momentum, eps, mu, rstd, scale, shift);
    return hipGetLastError();
}

hipError_t launch_tr_bnbwd_coef(const double* sums, int C, int64_t M, const float* gamma, const float* rstd, float* dgamma,
                                float* dbeta, float* k1, float* k2, float* k3, hipStream_t s) {
    hipLaunchKernelGGL(tr_bnbwd_coef_kernel, dim3((C + 127) / 128), dim3(128), 0, s, sums, C, M, gamma, rstd, dgamma, dbeta, k1,
                       k2, k3);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- BN backward, applied
// dz = k1[c] * (dy - k2[c] - xhat * k3[c]),  k1 = gamma*rstd, k2 = mean(dy), k3 = mean(dy*xhat)
// SEGSUM: the column sums of dz over each block's 128 rows as well (float64, a fixed order: a thread's rows in order,
// then the 16 row lanes in order), written to seg_part[blockIdx.y][C] — tr_blocksum_final_kernel adds a segment's blocks:
// the per-crop gradient of dconv1's per-crop term without a second pass over the 537 MB of dz (tr_segsum: 154 us).
template <bool DENSE, bool SEGSUM = false>
__global__ __launch_bounds__(256) void tr_bnbwd_apply_kernel(const float* __restrict__ z, int64_t M, int C, int64_t ldz,
                                                             DaSrc src, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ mu,
                                                             const float* __restrict__ rstd, const float* __restrict__ k1,
                                                             const float* __restrict__ k2, const float* __restrict__ k3,
                                                             float* __restrict__ dz, int64_t lddz, int cgs,
                                                             double* __restrict__ seg_part = nullptr,
                                                             uint32_t* __restrict__ amax = nullptr) {
    // block: 2^cgs groups of 4 channels x (256 >> cgs) rows, 128 rows in all; grid (C / (4 << cgs), M/128); cgs: tr_apply_cgs
    // (512-channel rows: a wave's 16-byte loads are 1 KiB of ONE row instead of 256-byte pieces of four rows, +4 %; the pass
    // runs at 5.3-5.6 TB/s either way — two streams in, one out). A thread walks its rows in batches of 8, all of a
    // batch's loads issued before the first is used (rows past the end are clamped for the loads and skipped for the stores).
    constexpr int U = 8;
    const int gl = threadIdx.x & ((1 << cgs) - 1), rl = threadIdx.x >> cgs, RP = 256 >> cgs;
    const int c = ((blockIdx.x << cgs) + gl) * 4;
    if (c >= C) return;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c), sh = *reinterpret_cast<const f32x4*>(shift + c);
    const f32x4 mean = *reinterpret_cast<const f32x4*>(mu + c), rs = *reinterpret_cast<const f32x4*>(rstd + c);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(k1 + c), a2 = *reinterpret_cast<const f32x4*>(k2 + c);
    const f32x4 a3 = *reinterpret_cast<const f32x4*>(k3 + c);
    double ssum[4] = {0.0, 0.0, 0.0, 0.0};                 // (SEGSUM; the host asks for it only when C % 64 == 0: no early return)
    uint32_t mx = 0;                                        // (amax: the bit pattern of the largest |dz| this thread wrote)
    for (int64_t pb = (int64_t)blockIdx.y * 128 + rl; pb < (int64_t)blockIdx.y * 128 + 128; pb += RP * U) {
        f32x4 v[U], d[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int64_t p = min(pb + RP * i, M - 1);
            v[i] = *reinterpret_cast<const f32x4*>(z + p * ldz + c);
            if (DENSE) {
                d[i] = *reinterpret_cast<const f32x4*>(src.da + p * src.ldda + c);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) d[i][e] = src.at(p, c + e, C);
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int64_t p = pb + RP * i;
            if (p >= M) break;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = v[i][e] * sc[e] + sh[e];
                const float dy = y > 0.0f ? d[i][e] : 0.0f;
                o[e] = a1[e] * (dy - a2[e] - (v[i][e] - mean[e]) * rs[e] * a3[e]);
            }
            *reinterpret_cast<f32x4*>(dz + p * lddz + c) = o;
            if (amax) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t b = __float_as_uint(o[e]) & 0x7fffffffu;
                    mx = b > mx ? b : mx;
                }
            }
            if (SEGSUM) {
#pragma unroll
                for (int e = 0; e < 4; ++e) ssum[e] += (double)o[e];
            }
        }
    }
    if (amax) {                                             // (C % 64 == 0: whole waves; one atomic per wave)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)mx, off);
            mx = other > mx ? other : mx;
        }
        // 64 words, a workgroup's by its index: 32,768 waves on ONE word are ~370 us of serialised atomics (88 per us).
        // Round 6: the four waves of the workgroup meet in LDS first and ONE atomic leaves per workgroup — the 64 words are
        // four 64-byte lines, and atomics on one line serialise at the memory side whatever the word: with an atomic per
        // wave this pass took 183 / 97 us at 256 / 128 channels x 262,144 rows against 139 / 66 us without the maximum
        // (profiles/r06_train_roofline_f16x3.json). (C % (4 << cgs) == 0 for every caller that asks for the maximum: no
        // thread has left at the top, the barrier is safe.)
        __shared__ uint32_t s_mx[4];
        if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t a = s_mx[0] > s_mx[1] ? s_mx[0] : s_mx[1], b = s_mx[2] > s_mx[3] ? s_mx[2] : s_mx[3];
            atomicMax(amax + ((blockIdx.y + 17u * blockIdx.x) & 63u), a > b ? a : b);
        }
    }
    if (SEGSUM) {                                           // a thread's rows in order (above), then the block's row lanes in order
        __shared__ double sm[1024];                         // [row lane][channel of the block]: RP x (4 << cgs) = 1024
        const int W = 4 << cgs;
#pragma unroll
        for (int e = 0; e < 4; ++e) sm[rl * W + gl * 4 + e] = ssum[e];
        __syncthreads();
        for (int cb = threadIdx.x; cb < W; cb += 256) {
            const int cc = blockIdx.x * W + cb;
            if (cc < C) {
                double t = 0.0;
                for (int i = 0; i < RP; ++i) t += sm[i * W + cb];
                seg_part[(int64_t)blockIdx.y * C + cc] = t;
            }
        }
    }
}

// threads per row (log2) of tr_bnbwd_apply_kernel: 512-channel strips where the rows are that long, else 64-channel strips
static int tr_apply_cgs(int C) {
#ifdef TR_APPLY_CGS
    return TR_APPLY_CGS;
#endif
    return C % 512 == 0 ? 7 : 4;        // (A/B at 262,144 rows: 512 channels 299 -> 287 us; 256 equal; 128 slower by 4 us as whole rows)
}

// out[s][c] = sum of the n_blk block partials of segment s, in block order (fp32 out)
__global__ __launch_bounds__(256) void tr_blocksum_final_kernel(const double* __restrict__ part, int n_blk, int C, int64_t n,
                                                                float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t s = i / C;
    const int c = (int)(i % C);
    double t = 0.0;
    for (int j = 0; j < n_blk; ++j) t += part[(s * n_blk + j) * C + c];
    out[i] = (float)t;
}

hipError_t launch_tr_bnbwd_apply(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                 const float* dg, const int32_t* arg, int64_t seg, const float* scale, const float* shift,
                                 const float* mu, const float* rstd, const float* k1, const float* k2, const float* k3,
                                 float* dz, int64_t lddz, hipStream_t s, uint32_t* amax) {
    DaSrc src{da, ldda, dg, arg, seg};
    const int cgs = tr_apply_cgs(C), W = 4 << cgs;
    const dim3 grid((C + W - 1) / W, (unsigned)((M + 127) / 128));
    if (da)
        hipLaunchKernelGGL((tr_bnbwd_apply_kernel<true>), grid, dim3(256), 0, s, z, M, C, ldz, src, scale, shift, mu, rstd, k1,
                           k2, k3, dz, lddz, cgs, nullptr, amax);
    else
        hipLaunchKernelGGL((tr_bnbwd_apply_kernel<false>), grid, dim3(256), 0, s, z, M, C, ldz, src, scale, shift, mu, rstd, k1,
                           k2, k3, dz, lddz, cgs, nullptr, amax);
    return hipGetLastError();
}

// the same with the per-segment column sums of dz: sum_seg % 128 == 0, M % sum_seg == 0, C % 64 == 0, dense da
size_t tr_bnbwd_apply_segsum_workspace_bytes(int64_t M, int C) { return (size_t)((M + 127) / 128) * C * sizeof(double); }
hipError_t launch_tr_bnbwd_apply_segsum(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                        const float* scale, const float* shift, const float* mu, const float* rstd,
                                        const float* k1, const float* k2, const float* k3, float* dz, int64_t lddz,
                                        int64_t sum_seg, float* seg_sums, double* ws, hipStream_t s) {
    DaSrc src{da, ldda, nullptr, nullptr, 0};
    const int cgs = tr_apply_cgs(C), W = 4 << cgs;
    const dim3 grid((C + W - 1) / W, (unsigned)((M + 127) / 128));
    hipLaunchKernelGGL((tr_bnbwd_apply_kernel<true, true>), grid, dim3(256), 0, s, z, M, C, ldz, src, scale, shift, mu, rstd, k1, k2,
                       k3, dz, lddz, cgs, ws);
    const int64_t n = (M / sum_seg) * C;
    hipLaunchKernelGGL(tr_blocksum_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws, (int)(sum_seg / 128), C, n,
                       seg_sums);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- wgrad
// dW[co][ci] = sum_p dz[p][co] * act(a[p][ci]): D(32 co x 32 ci) += A(co x 2 points) . B(2 points x ci) per MFMA.
// A lane (co = lane&31, h) reads dz[p0 + 2s + h][co], B lane (ci, h) reads a[p0 + 2s + h][ci]: each a 128-B row
// segment per half-wave. A wave owns a WG_MT x WG_KT block of tiles and a slice of the points; the slices' partial
// sums go to part[slice][co][ci] and are added in slice order by tr_wgrad_final_kernel (deterministic).
#define WG_MT 4
#define WG_KT 2
#define WG_MIN_SLICE 128                 // fewest points per wave
#define WG_KS 8                           // k-steps (pairs of points) per operand block

template <int MT, int KT>
struct WgBlock {
    float av[WG_KS][MT], bv[WG_KS][KT];
};

// pa / pb point at this lane's element of the block's first point row: dz[(p0 + h)][32*mt0 + m], a[(p0 + h)][32*kt0 + m];
// the tiles of the block are 32 floats apart, successive k-steps two rows apart. A tile past the layer's edge (t >= n_mt,
// k >= n_kt) re-reads the last real one — oa / ob hold the clamped offsets — and its accumulator is simply never stored:
// a conditional load (`t < n_mt ? p[..] : 0`) is a BRANCH per load to hipcc, 50-120 of them per 16-point block, and
// with them every load, its address arithmetic and the activation sat in one blob between two bursts of MFMAs (the big
// layers ran at 58 % of peak for it).
// FULL: every tile of the block is real (c_out % (32 MT) == 0 and c_in % (32 KT) == 0: all the big layers) — the tile
// offsets are then compile-time constants and travel in the load's immediate field: ONE 64-bit address per k-step and
// operand instead of one per load (round 4: 144 of the 246 vector instructions of the <4, 4, 2> loop body were
// v_lshl_add_u64, beside 128 MFMAs that share the SIMD's FMA lanes with them: tools/isa_mix.py, tools/pmc_train.sh).
template <bool FULL, int MT, int KT>
__device__ __forceinline__ void wg_load(WgBlock<MT, KT>& bk, const float* __restrict__ pa, int64_t lddz,
                                        const float* __restrict__ pb, int64_t lda, const int (&oa)[MT], const int (&ob)[KT]) {
#pragma unroll
    for (int s = 0; s < WG_KS; ++s) {
        const float* ra = pa + 2 * s * lddz;
        const float* rb = pb + 2 * s * lda;
#pragma unroll
        for (int t = 0; t < MT; ++t) bk.av[s][t] = ra[FULL ? 32 * t : oa[t]];
#pragma unroll
        for (int k = 0; k < KT; ++k) bk.bv[s][k] = rb[FULL ? 32 * k : ob[k]];        // raw; activation at use
    }
}

template <int MT, int KT>
__device__ __forceinline__ void wg_compute(WgBlock<MT, KT>& bk, f32x16 (&acc)[MT][KT], const float (&sc)[KT],
                                           const float (&sh)[KT], bool act, int relu_in) {
    if (act) {
#pragma unroll
        for (int s = 0; s < WG_KS; ++s)
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float v = bk.bv[s][k] * sc[k] + sh[k];
                bk.bv[s][k] = relu_in ? fmaxf(v, 0.0f) : v;
            }
    }
#pragma unroll
    for (int s = 0; s < WG_KS; ++s)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int k = 0; k < KT; ++k) acc[t][k] = mfma32(bk.av[s][t], bk.bv[s][k], acc[t][k]);
}

// MT x KT: the block of tiles a wave owns; NB: operand blocks (16 points each) in its ring — NB - 1 are in flight while
// one is consumed. The big layers run <4, 2, 2> (128 accumulator registers, 96 of operands); layers with at most 64
// output channels would leave most of that idle and are bound by the latency of their loads instead (one 16-point block
// in flight per wave: 93 us for 134 MB), so they run <2, 2, 4>: three blocks in flight in the same registers (55 us).
// COMB: the four waves of a workgroup take four consecutive slices of ONE tile block and add their tiles through LDS before
// anything is written (see below). Not for the 4 x 4-tile variant: its waves then stop sharing operand rows in L1 and its
// 256 accumulator registers spill around the exchange (A/B, both orders: 512 x 256 +2–3 %, the small layers −5…−10 %).
template <int MT, int KT, int NB, bool FULL = false, bool COMB = false>
__global__ __launch_bounds__(256) void tr_wgrad_kernel(const float* __restrict__ dz, int64_t lddz, const float* __restrict__ a,
                                                       int64_t lda, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int relu_in, int64_t M, int c_out,
                                                       int c_in, float* __restrict__ part, int n_mb, int n_kb,
                                                       int64_t slice_pts) {
    const int lane = threadIdx.x & 63, h = lane >> 5, m = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // COMB: a quarter of the partial sums in memory (round 4: 235 MB of slices written and read back per step —
    // `tools/pmc_train_traffic.sh` — beside 4 GB of operands). A tail wave computes nothing and joins the reduction with zeros.
    const int64_t unit = (int64_t)blockIdx.x * 4 + wave;
    const int blk = COMB ? (int)(blockIdx.x % (unsigned)(n_mb * n_kb)) : (int)(unit % (n_mb * n_kb));
    const int64_t slice_out = COMB ? blockIdx.x / (unsigned)(n_mb * n_kb) : unit / (n_mb * n_kb);
    const int64_t slice = COMB ? slice_out * 4 + wave : slice_out;
    const bool idle = slice * slice_pts >= M;
    if (!COMB && idle) return;
    const int64_t p_begin = idle ? 0 : slice * slice_pts;
    const int64_t p_end = idle ? 0 : min(M, p_begin + slice_pts);  // M % 32 == 0, slice_pts % 64 == 0: whole 16-point blocks
    const int mt0 = (blk / n_kb) * MT, kt0 = (blk % n_kb) * KT;
    const int n_mt = min(MT, c_out / 32 - mt0), n_kt = min(KT, c_in / 32 - kt0);
    int oa[MT], ob[KT];                                        // tile offsets, clamped to the last real tile (see wg_load)
#pragma unroll
    for (int t = 0; t < MT; ++t) oa[t] = 32 * min(t, n_mt - 1);
#pragma unroll
    for (int k = 0; k < KT; ++k) ob[k] = 32 * min(k, n_kt - 1);
    float sc[KT], sh[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        sc[k] = scale ? scale[32 * kt0 + ob[k] + m] : 1.0f;
        sh[k] = scale ? shift[32 * kt0 + ob[k] + m] : 0.0f;
    }
    f32x16 acc[MT][KT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[t][k] = f32x16{};
    const bool act = scale != nullptr;
    WgBlock<MT, KT> ring[NB];
    const float* const pa0 = dz + (p_begin + h) * lddz + 32 * mt0 + m;
    const float* const pb0 = a + (p_begin + h) * lda + 32 * kt0 + m;
    const int64_t sa = 2 * WG_KS * lddz, sb = 2 * WG_KS * lda;
    // steady state without data-dependent branches around the loads: a load past the slice's end re-reads the slice's
    // first block (valid memory, values unused) instead of being skipped
    const int64_t n_blk = (p_end - p_begin) / (2 * WG_KS);
    if constexpr (NB == 2) {
        // ping-pong with running pointers (n_blk is even: M and the slices are multiples of 32 points)
        const float* pa = pa0;
        const float* pb = pb0;
        wg_load<FULL>(ring[0], pa, lddz, pb, lda, oa, ob);
        for (int64_t i = 0; i < n_blk; i += 2) {
            wg_load<FULL>(ring[1], pa + sa, lddz, pb + sb, lda, oa, ob);
            DAL3_SCHED_FENCE();
            wg_compute(ring[0], acc, sc, sh, act, relu_in);
            DAL3_SCHED_FENCE();
            const bool more = i + 2 < n_blk;
            pa = more ? pa + 2 * sa : pa0;
            pb = more ? pb + 2 * sb : pb0;
            wg_load<FULL>(ring[0], pa, lddz, pb, lda, oa, ob);
            DAL3_SCHED_FENCE();
            wg_compute(ring[1], acc, sc, sh, act, relu_in);
            DAL3_SCHED_FENCE();
        }
    } else {
        // NB blocks: the slice is padded to a multiple of NB blocks by the same re-read, the surplus computes are
        // skipped (wave-uniform)
#pragma unroll
        for (int b = 0; b < NB - 1; ++b) {
            const int64_t i = b < n_blk ? b : 0;
            wg_load<FULL>(ring[b], pa0 + i * sa, lddz, pb0 + i * sb, lda, oa, ob);
        }
        for (int64_t i0 = 0; i0 < n_blk; i0 += NB) {
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int64_t nx = i0 + u + NB - 1;
                const int64_t j = nx < n_blk ? nx : 0;
                wg_load<FULL>(ring[(u + NB - 1) % NB], pa0 + j * sa, lddz, pb0 + j * sb, lda, oa, ob);
                DAL3_SCHED_FENCE();
                if (i0 + u < n_blk) wg_compute(ring[u], acc, sc, sh, act, relu_in);
                DAL3_SCHED_FENCE();
            }
        }
    }
    if constexpr (COMB) {
        // waves 1..3 hand their tiles to wave 0, four tiles at a time (48 KiB of LDS), added in wave order: a fixed association
        __shared__ float comb[3][4][16][64];
        constexpr int NT = MT * KT;
#pragma unroll
        for (int g0 = 0; g0 < NT; g0 += 4) {
            if (wave > 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (g0 + u < NT) comb[wave - 1][u][r][lane] = acc[(g0 + u) / KT][(g0 + u) % KT][r];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int w = 0; w < 3; ++w)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (g0 + u < NT) acc[(g0 + u) / KT][(g0 + u) % KT][r] += comb[w][u][r][lane];
            }
            __syncthreads();
        }
        if (wave != 0) return;
    }
    // D tile: row (co) = tile_chan(r, h), col (ci) = lane & 31
    float* out = part + slice_out * (int64_t)c_out * c_in;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        if (t >= n_mt) break;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (k >= n_kt) break;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[(int64_t)(32 * (mt0 + t) + tile_chan(r, h)) * c_in + 32 * (kt0 + k) + m] = acc[t][k][r];
        }
    }
}

// 64 elements x WGF_L slice-lanes per block; lane l adds slices l, l + L, ... (four interleaved chains), then the L lane
// sums are added in lane order: a fixed association. (Round 4: 16 lanes, was 4 — the 64-channel layers have 1024 slices,
// which four lanes walked in 64 dependent trips: 20 us, seventeen times a step.)
#ifndef WGF_L
#define WGF_L 16
#endif
__device__ __forceinline__ void wgrad_final_block(const float* __restrict__ part, int n_slices, int64_t n, float* __restrict__ dW,
                                                  uint32_t block, float (*sm)[64]) {
    const int el = threadIdx.x & 63, l = threadIdx.x >> 6;
    const int64_t i = (int64_t)block * 64 + el;
    float s = 0.0f;
    if (i < n) {
        float u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f;       // four independent chains: the loop is load-latency bound
        int k = l;
        for (; k + 3 * WGF_L < n_slices; k += 4 * WGF_L) {
            u0 += part[(int64_t)k * n + i];
            u1 += part[(int64_t)(k + WGF_L) * n + i];
            u2 += part[(int64_t)(k + 2 * WGF_L) * n + i];
            u3 += part[(int64_t)(k + 3 * WGF_L) * n + i];
        }
        for (; k < n_slices; k += WGF_L) u0 += part[(int64_t)k * n + i];
        s = (u0 + u1) + (u2 + u3);
    }
    sm[l][el] = s;
    __syncthreads();
    if (l == 0 && i < n) {
        float t = sm[0][el];
#pragma unroll
        for (int j = 1; j < WGF_L; ++j) t += sm[j][el];
        dW[i] = t;
    }
}
__global__ __launch_bounds__(64 * WGF_L) void tr_wgrad_final_kernel(const float* __restrict__ part, int n_slices, int64_t n,
                                                                   float* __restrict__ dW) {
    __shared__ float sm[WGF_L][64];
    wgrad_final_block(part, n_slices, n, dW, blockIdx.x, sm);
}

// slice length: enough (tile block, slice) units to occupy the chip (~1024 waves: with 2048 the partial sums of the
// small layers — one (c_out x c_in) tile block per 128 points — were a quarter of the traffic, and every shape ran 5-20 %
// slower) without going below WG_MIN_SLICE points per wave; a multiple of 64
static bool wgrad_small(int c_out) { return c_out <= 64; }    // at most two out-tiles: the <2, 2, 4> instantiation
#ifndef WG_BIG_KT
#define WG_BIG_KT 4
#endif
// in-tiles per wave: 4 x 4 tiles for the biggest layers (16 MFMAs per 8 operand loads instead of 8 per 6: without its
// loads the 512 x 256 wgrad takes 483 us instead of 611, and what the loads cost is L2 -> CU traffic, every dz tile being
// read once per block of in-tiles: 582 -> 555 us). Smaller layers have too few blocks for it (128 x 128: 101 -> 114 us).
static int wgrad_kt(int c_out, int c_in) { return (c_out % 128 == 0 && c_in % 128 == 0 && c_out >= 256 && c_in >= 256) ? WG_BIG_KT : WG_KT; }
static void wgrad_blocks(int c_out, int c_in, int* n_mb, int* n_kb) {
    const int mt = wgrad_small(c_out) ? 2 : WG_MT;
    *n_mb = (c_out / 32 + mt - 1) / mt;
    const int kt = wgrad_kt(c_out, c_in);
    *n_kb = (c_in / 32 + kt - 1) / kt;
}
static int64_t wgrad_slice_pts(int64_t M, int c_out, int c_in) {
    int n_mb, n_kb;
    wgrad_blocks(c_out, c_in, &n_mb, &n_kb);
    const int64_t blocks = (int64_t)n_mb * n_kb;
    const int64_t want_slices = (1024 + blocks - 1) / blocks;
    int64_t pts = (M + want_slices - 1) / want_slices;
    pts = (pts + 63) / 64 * 64;
    return pts < WG_MIN_SLICE ? WG_MIN_SLICE : pts;
}

// partial sums in memory: one per workgroup (its four waves' slices added through LDS: tr_wgrad_kernel COMB) or one per wave
static bool wgrad_comb(int c_out, int c_in) { return wgrad_small(c_out) || wgrad_kt(c_out, c_in) != 4; }
static int64_t wgrad_out_slices(int64_t M, int64_t pts, bool comb) {
    const int64_t n = (M + pts - 1) / pts;
    return comb ? (n + 3) / 4 : n;
}
size_t tr_wgrad_workspace_bytes(int64_t M, int c_out, int c_in) {
    const int64_t pts = wgrad_slice_pts(M, c_out, c_in);
    return (size_t)wgrad_out_slices(M, pts, wgrad_comb(c_out, c_in)) * c_out * c_in * sizeof(float);
}

// The second stages of SEVERAL weight gradients in one launch (round 4: a backward pass issued one 5-us second stage behind
// each of its 10–14 wgrad kernels; nothing reads a dW before the optimizer, so they can all wait for the end of the
// backward function). Same kernel body and association as tr_wgrad_final_kernel; the table travels in the kernel arguments.
#define TR_FINAL_MAX 24
struct TrFinalItem {
    const float* part;
    float* dW;
    int64_t n;
    int32_t n_slices;
    uint32_t first_block;                                   // of 64 elements; blocks [first_block, next item's) belong to it
};
struct TrFinalMany {
    TrFinalItem it[TR_FINAL_MAX];
    int n;
};
__global__ __launch_bounds__(64 * WGF_L) void tr_wgrad_final_many_kernel(TrFinalMany p) {
    __shared__ float sm[WGF_L][64];
    int k = 0;
    for (int i = 1; i < p.n; ++i) k = blockIdx.x >= p.it[i].first_block ? i : k;      // (first_block is ascending)
    const TrFinalItem& t = p.it[k];
    wgrad_final_block(t.part, t.n_slices, t.n, t.dW, blockIdx.x - t.first_block, sm);
}
hipError_t launch_tr_wgrad_final_many(const dal3_tr_wgrad_part* items, int n, hipStream_t s) {
    if (n <= 0 || n > TR_FINAL_MAX) return hipErrorInvalidValue;
    TrFinalMany p;
    p.n = n;
    uint32_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        p.it[i] = TrFinalItem{items[i].part, items[i].dW, items[i].n, (int32_t)items[i].n_slices, blocks};
        blocks += (uint32_t)((items[i].n + 63) / 64);
    }
    hipLaunchKernelGGL(tr_wgrad_final_many_kernel, dim3(blocks), dim3(64 * WGF_L), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tr_wgrad_final(const float* part, int n_slices, int64_t n, float* dW, hipStream_t s) {
    hipLaunchKernelGGL(tr_wgrad_final_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * WGF_L), 0, s, part, n_slices, n, dW);
    return hipGetLastError();
}

hipError_t launch_tr_wgrad(const float* dz, int64_t lddz, const float* a, int64_t lda, const float* scale,
                           const float* shift, int relu_in, int64_t M, int c_out, int c_in, float* part, float* dW,
                           hipStream_t s) {
    int n_mb, n_kb;
    wgrad_blocks(c_out, c_in, &n_mb, &n_kb);
    const int64_t pts = wgrad_slice_pts(M, c_out, c_in);
    const bool comb = wgrad_comb(c_out, c_in);
    const int64_t n_slices = wgrad_out_slices(M, pts, comb);    // as they reach memory
    const dim3 grid(comb ? (unsigned)(n_slices * n_mb * n_kb) : (unsigned)((n_slices * n_mb * n_kb + 3) / 4));
    // whole blocks take the compile-time tile offsets (FULL; against the clamped-offset loads: profiles/LEDGER_r04.md 2.1 item 10);
    // wgrad_comb is the one place that decides COMB (both kinds of every shape stay instantiated)
    const auto go = [&](auto plain, auto full, int mt, int kt) {
        if (c_out % (32 * mt) == 0 && c_in % (32 * kt) == 0)
            hipLaunchKernelGGL(full, grid, dim3(256), 0, s, dz, lddz, a, lda, scale, shift, relu_in, M, c_out, c_in, part, n_mb, n_kb, pts);
        else
            hipLaunchKernelGGL(plain, grid, dim3(256), 0, s, dz, lddz, a, lda, scale, shift, relu_in, M, c_out, c_in, part, n_mb, n_kb, pts);
    };
    if (wgrad_small(c_out)) {
        if (comb) go(tr_wgrad_kernel<2, WG_KT, 4, false, true>, tr_wgrad_kernel<2, WG_KT, 4, true, true>, 2, WG_KT);
        else go(tr_wgrad_kernel<2, WG_KT, 4>, tr_wgrad_kernel<2, WG_KT, 4, true>, 2, WG_KT);
    } else if (wgrad_kt(c_out, c_in) == 4) {
        go(tr_wgrad_kernel<WG_MT, 4, 2>, tr_wgrad_kernel<WG_MT, 4, 2, true>, WG_MT, 4);
    } else {
        if (comb) go(tr_wgrad_kernel<WG_MT, WG_KT, 2, false, true>, tr_wgrad_kernel<WG_MT, WG_KT, 2, true, true>, WG_MT, WG_KT);
        else go(tr_wgrad_kernel<WG_MT, WG_KT, 2>, tr_wgrad_kernel<WG_MT, WG_KT, 2, true>, WG_MT, WG_KT);
    }
    if (!dW) return hipGetLastError();                          // the caller adds the slices later (dal3_tr_wgrad_final_many)
    const int64_t n = (int64_t)c_out * c_in;
    hipLaunchKernelGGL(tr_wgrad_final_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * WGF_L), 0, s, part, (int)n_slices, n, dW);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- activation + Dropout
// out[p][c] = act(x[p][c]) * m[p][c],  m = mult[p][c] when given, else (keep ? 1/(1-p) : 0) with keep drawn by a
// counter-based generator keyed on (seed + step, p*C + c): the backward pass re-creates the same multiplier from the
// same key instead of reading a stored (M x C) mask (128 MB at 64 x 4096 points for ins_seg's Dropout), and `step`
// is read from DEVICE memory so that a step captured into a hipGraph draws afresh on every replay (the host bumps
// that scalar with an ordinary captured op). 16 bytes per lane, rows of C floats (C a multiple of 4).
// One draw per FOUR consecutive elements (a lane's 16 bytes): the splitmix64 finaliser of (key, index of the quad), its 64 bits
// cut into four 16-bit fields, element e kept when field e >= thresh (thresh = p_drop * 65536: the keep probability is exact
// to 2^-16; p = 0.5 exactly). Round 4: one 64-bit hash per ELEMENT — ~28 vector instructions each — made the three kernels of
// the logits layer compute-bound at 3.1–4.7 TB/s (`profiles/r04_train_traffic.txt`); every kernel that re-creates the multiplier
// calls this one function.
__device__ __forceinline__ uint64_t tr_hash_quad(uint64_t key, uint64_t quad) {
    uint64_t z = key + quad * 0x9E3779B97F4A7C15ull;                    // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ bool tr_keep(uint64_t h, int e, uint32_t thresh) { return (uint32_t)((h >> (16 * e)) & 0xffffu) >= thresh; }
static uint32_t tr_drop_thresh(float p_drop) {                          // 0 (keep everything, no draw) .. 65536 (keep nothing)
    if (p_drop <= 0.0f) return 0u;
    const double t = (double)p_drop * 65536.0 + 0.5;
    return t >= 65536.0 ? 65536u : (uint32_t)t;
}
__global__ __launch_bounds__(256) void tr_act_dropout_kernel(const float* __restrict__ x, int64_t M, int C, int64_t ldx,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             int relu, const float* __restrict__ mult, int64_t ldm,
                                                             uint64_t seed, const int64_t* __restrict__ step, uint32_t thresh,
                                                             float keep_scale, float* __restrict__ out, int64_t ldo) {
    const int c4 = C / 4;
    const int64_t n = M * c4, stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t key = seed + (step ? (uint64_t)(*step) * 0xD1B54A32D192ED03ull : 0ull);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t p = i / c4;
        const int c = (int)(i - p * c4) * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(x + p * ldx + c);
        if (scale) {
            const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c), sh = *reinterpret_cast<const f32x4*>(shift + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(v[e], sc[e], sh[e]);
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
        }
        if (mult) {
            const f32x4 mv = *reinterpret_cast<const f32x4*>(mult + p * ldm + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= mv[e];
        } else if (thresh != 0u) {                          // (p_drop == 0: every element kept at scale 1, no draw to make)
            const uint64_t hq = tr_hash_quad(key, (uint64_t)(p * C + c) >> 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = tr_keep(hq, e, thresh) ? v[e] * keep_scale : 0.0f;
        }
        *reinterpret_cast<f32x4*>(out + p * ldo + c) = v;
    }
}
hipError_t launch_tr_act_dropout(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift, int relu,
                                 const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop, float* out,
                                 int64_t ldo, hipStream_t s) {
    const int64_t n = M * (C / 4);
    const int64_t want = (n + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
    const uint32_t thresh = tr_drop_thresh(p_drop);
    const float keep_scale = p_drop < 1.0f ? 1.0f / (1.0f - p_drop) : 0.0f;
    hipLaunchKernelGGL(tr_act_dropout_kernel, dim3(grid), dim3(256), 0, s, x, M, C, ldx, scale, shift, relu, mult, ldm, seed, step,
                       thresh, keep_scale, out, ldo);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the 128 -> 2 logits layer
// dconv5 is Dropout(relu(dbn4(z4))) -> Conv1d(128, 2) (static_model.py:292-294). Through the MFMA kernels it was the
// activation + Dropout pass writing a4 (134 MB), a 128 -> 32 linear on a weight padded from 2 to 32 rows, and backward a
// zero-padded (M, 32) gradient, a 32 -> 128 dgrad, the Dropout pass over its output and a 32 x 128 wgrad: 0.30 ms of a
// 7.1 ms step for 512 multiply-adds per point. Three VALU kernels instead (round 4), a4 never materialised — the
// multiplier is re-created from its key wherever it is needed, exactly as tr_act_dropout_kernel draws it:
//   forward  logits[p][j] = b[j] + sum_c W[j][c] * m[p][c] * act(z[p][c])
//   dgrad    da[p][c]     = m[p][c] * (dl[p][0] W[0][c] + dl[p][1] W[1][c])          (gradient w.r.t. act(z), Dropout undone)
//   wgrad    dW[j][c]     = sum_p dl[p][j] * m[p][c] * act(z[p][c]),  db[j] = sum_p dl[p][j]   (float64 partials per 256 rows,
//            added in row-block order by tr_colred_final_kernel<0>: the column-reduction machinery, MODE 2)
// 32 lanes x 4 channels per point: C == 128.
struct DropKey {
    const float* mult;                   // explicit multiplier (M x C, row stride ldm) or NULL
    int64_t ldm;
    uint64_t key;                        // seed + step * const (resolved on the device: step lives there)
    uint32_t thresh;
    float keep_scale;
};
__device__ __forceinline__ f32x4 drop_mult4(const DropKey& d, int64_t p, int c, int C) {
    if (d.mult) return *reinterpret_cast<const f32x4*>(d.mult + p * d.ldm + c);
    if (d.thresh == 0u) return f32x4{d.keep_scale, d.keep_scale, d.keep_scale, d.keep_scale};      // p_drop == 0: no draw
    f32x4 m;
    const uint64_t hq = tr_hash_quad(d.key, (uint64_t)(p * C + c) >> 2);
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = tr_keep(hq, e, d.thresh) ? d.keep_scale : 0.0f;
    return m;
}
__device__ __forceinline__ f32x4 act4(const f32x4 v, const f32x4 sc, const f32x4 sh, bool affine, int relu) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = affine ? __builtin_fmaf(v[e], sc[e], sh[e]) : v[e];
        o[e] = relu ? fmaxf(x, 0.0f) : x;
    }
    return o;
}
__global__ __launch_bounds__(256) void tr_head2_fwd_kernel(const float* __restrict__ z, int64_t M, int64_t ldz,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, int relu,
                                                           DropKey d, uint64_t seed, const int64_t* __restrict__ step,
                                                           const float* __restrict__ W, int64_t ldw, const float* __restrict__ bias,
                                                           float* __restrict__ logits) {
    constexpr int C = 128;
    const int l = threadIdx.x & 31, c = 4 * l;
    d.key = seed + (step ? (uint64_t)(*step) * 0xD1B54A32D192ED03ull : 0ull);
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(W + c), w1 = *reinterpret_cast<const f32x4*>(W + ldw + c);
    f32x4 sc = {1, 1, 1, 1}, sh = {0, 0, 0, 0};
    if (scale) {
        sc = *reinterpret_cast<const f32x4*>(scale + c);
        sh = *reinterpret_cast<const f32x4*>(shift + c);
    }
    const float b0 = bias[0], b1 = bias[1];
    const int64_t stride = (int64_t)gridDim.x * 8;
    for (int64_t p0 = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5); p0 < M; p0 += 4 * stride) {
        f32x4 v[4];                                         // four points' loads in flight per lane group
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(z + min(p0 + u * stride, M - 1) * ldz + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + u * stride;
            if (p >= M) break;                              // (uniform over the 32 lanes of a point)
            const f32x4 a = act4(v[u], sc, sh, scale != nullptr, relu), m = drop_mult4(d, p, c, C);
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = a[e] * m[e];
                s0 = __builtin_fmaf(x, w0[e], s0);
                s1 = __builtin_fmaf(x, w1[e], s1);
            }
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) {             // a fixed tree over the point's 32 lanes
                s0 += __shfl_xor(s0, o, 64);
                s1 += __shfl_xor(s1, o, 64);
            }
            if (l == 0) {
                f32x2 o2 = {s0 + b0, s1 + b1};
                *reinterpret_cast<f32x2*>(logits + p * 2) = o2;
            }
        }
    }
}
__global__ __launch_bounds__(256) void tr_head2_dgrad_kernel(const float* __restrict__ dl, int64_t M, DropKey d, uint64_t seed,
                                                             const int64_t* __restrict__ step, const float* __restrict__ W,
                                                             int64_t ldw, float* __restrict__ da, int64_t ldda) {
    constexpr int C = 128;
    const int l = threadIdx.x & 31, c = 4 * l;
    d.key = seed + (step ? (uint64_t)(*step) * 0xD1B54A32D192ED03ull : 0ull);
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(W + c), w1 = *reinterpret_cast<const f32x4*>(W + ldw + c);
    const int64_t stride = (int64_t)gridDim.x * 8;
    for (int64_t p = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5); p < M; p += stride) {
        const f32x2 g = *reinterpret_cast<const f32x2*>(dl + p * 2);
        const f32x4 m = drop_mult4(d, p, c, C);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = m[e] * __builtin_fmaf(g[0], w0[e], g[1] * w1[e]);
        *reinterpret_cast<f32x4*>(da + p * ldda + c) = o;
    }
}
// dgrad TOGETHER with the BatchNorm-backward sums of the layer below (dbn4): the thread that forms da[p][c] also reads that
// layer's pre-BN value, gates it and accumulates sum dy, sum dy * xhat for its four channels (float64, as tr_colred_kernel
// mode 1; one partial row per 256-row block, added by tr_colred_final_kernel<2> with the coefficient epilogue) — the
// separate sums pass (a read of da and z: 60 us) becomes one more read of z inside this HBM-bound kernel.
__global__ __launch_bounds__(256) void tr_head2_dgrad_sums_kernel(const float* __restrict__ dl, int64_t M, DropKey d, uint64_t seed,
                                                                  const int64_t* __restrict__ step, const float* __restrict__ W,
                                                                  int64_t ldw, float* __restrict__ da, int64_t ldda,
                                                                  const float* __restrict__ bz, int64_t ldbz,
                                                                  const float* __restrict__ bscale, const float* __restrict__ bshift,
                                                                  const float* __restrict__ bmu, const float* __restrict__ brstd,
                                                                  double* __restrict__ part) {
    constexpr int C = 128;
    __shared__ double sm[2][8][C];
    const int l = threadIdx.x & 31, rl = threadIdx.x >> 5, c = 4 * l;
    d.key = seed + (step ? (uint64_t)(*step) * 0xD1B54A32D192ED03ull : 0ull);
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(W + c), w1 = *reinterpret_cast<const f32x4*>(W + ldw + c);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(bscale + c), sh = *reinterpret_cast<const f32x4*>(bshift + c);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(bmu + c), rs = *reinterpret_cast<const f32x4*>(brstd + c);
    const int64_t r0 = (int64_t)blockIdx.x * TR_RED_ROWS, r1 = min(M, r0 + TR_RED_ROWS);
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    for (int64_t p0 = r0 + rl; p0 < r1; p0 += 8 * 4) {
        f32x4 v[4];
        f32x2 g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = min(p0 + 8 * u, M - 1);
            v[u] = *reinterpret_cast<const f32x4*>(bz + p * ldbz + c);
            g[u] = *reinterpret_cast<const f32x2*>(dl + p * 2);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + 8 * u;
            if (p >= r1) break;
            const f32x4 m = drop_mult4(d, p, c, C);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = m[e] * __builtin_fmaf(g[u][0], w0[e], g[u][1] * w1[e]);
                const float y = v[u][e] * sc[e] + sh[e];
                const float dy = y > 0.0f ? o[e] : 0.0f;
                s0[e] += dy;
                s1[e] += (double)dy * ((v[u][e] - mu[e]) * rs[e]);
            }
            *reinterpret_cast<f32x4*>(da + p * ldda + c) = o;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sm[0][rl][c + e] = s0[e];
        sm[1][rl][c + e] = s1[e];
    }
    __syncthreads();
    if (threadIdx.x < C) {
        double a0 = 0.0, a1 = 0.0;
        for (int i = 0; i < 8; ++i) {
            a0 += sm[0][i][threadIdx.x];
            a1 += sm[1][i][threadIdx.x];
        }
        const int64_t o = ((int64_t)blockIdx.x * C + threadIdx.x) * 2;
        part[o] = a0;
        part[o + 1] = a1;
    }
}
// wgrad: per block 256 rows x 128 channels (+ the two bias sums in channel slots 128, 129): thread = (4 channels, 8 row
// lanes), float64 partial sums, one partial row per block — the layout tr_colred_final_kernel<0> adds up (C = 130 columns)
#define H2_COLS 130
__global__ __launch_bounds__(256) void tr_head2_wgrad_kernel(const float* __restrict__ dl, const float* __restrict__ z, int64_t M,
                                                             int64_t ldz, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int relu, DropKey d, uint64_t seed,
                                                             const int64_t* __restrict__ step, double* __restrict__ part) {
    constexpr int C = 128;
    __shared__ double sm[2][8][H2_COLS];
    const int l = threadIdx.x & 31, rl = threadIdx.x >> 5, c = 4 * l;
    d.key = seed + (step ? (uint64_t)(*step) * 0xD1B54A32D192ED03ull : 0ull);
    f32x4 sc = {1, 1, 1, 1}, sh = {0, 0, 0, 0};
    if (scale) {
        sc = *reinterpret_cast<const f32x4*>(scale + c);
        sh = *reinterpret_cast<const f32x4*>(shift + c);
    }
    const int64_t r0 = (int64_t)blockIdx.x * TR_RED_ROWS, r1 = min(M, r0 + TR_RED_ROWS);
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, t0 = 0.0, t1 = 0.0;
    for (int64_t p0 = r0 + rl; p0 < r1; p0 += 8 * 4) {
        f32x4 v[4];
        f32x2 g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = min(p0 + 8 * u, M - 1);
            v[u] = *reinterpret_cast<const f32x4*>(z + p * ldz + c);
            g[u] = *reinterpret_cast<const f32x2*>(dl + p * 2);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + 8 * u;
            if (p >= r1) break;
            const f32x4 a = act4(v[u], sc, sh, scale != nullptr, relu), m = drop_mult4(d, p, c, C);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double x = (double)(a[e] * m[e]);
                s0[e] += x * (double)g[u][0];
                s1[e] += x * (double)g[u][1];
            }
            if (l == 0) {
                t0 += (double)g[u][0];
                t1 += (double)g[u][1];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sm[0][rl][c + e] = s0[e];
        sm[1][rl][c + e] = s1[e];
    }
    if (l == 0) {
        sm[0][rl][128] = t0;                                // db[0]: column 128 of "sum 0", db[1]: column 129
        sm[0][rl][129] = t1;
        sm[1][rl][128] = 0.0;
        sm[1][rl][129] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < H2_COLS) {
        double a0 = 0.0, a1 = 0.0;
        for (int i = 0; i < 8; ++i) {
            a0 += sm[0][i][threadIdx.x];
            a1 += sm[1][i][threadIdx.x];
        }
        const int64_t o = ((int64_t)blockIdx.x * H2_COLS + threadIdx.x) * 2;
        part[o] = a0;
        part[o + 1] = a1;
    }
}
static DropKey drop_key(const float* mult, int64_t ldm, float p_drop) {
    DropKey d{};
    d.mult = mult, d.ldm = ldm;
    d.thresh = tr_drop_thresh(p_drop);
    d.keep_scale = p_drop < 1.0f ? 1.0f / (1.0f - p_drop) : 0.0f;
    return d;
}
static unsigned head2_grid(int64_t M) {
    const int64_t want = (M + 7) / 8;
    return (unsigned)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
}
hipError_t launch_tr_head2_forward(const float* z, int64_t M, int64_t ldz, const float* scale, const float* shift, int relu,
                                   const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop, const float* W,
                                   int64_t ldw, const float* bias, float* logits, hipStream_t s) {
    hipLaunchKernelGGL(tr_head2_fwd_kernel, dim3(head2_grid((M + 3) / 4)), dim3(256), 0, s, z, M, ldz, scale, shift, relu,
                       drop_key(mult, ldm, p_drop), seed, step, W, ldw, bias, logits);
    return hipGetLastError();
}
hipError_t launch_tr_head2_dgrad(const float* dl, int64_t M, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step,
                                 float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda, hipStream_t s) {
    hipLaunchKernelGGL(tr_head2_dgrad_kernel, dim3(head2_grid(M)), dim3(256), 0, s, dl, M, drop_key(mult, ldm, p_drop), seed, step, W,
                       ldw, da, ldda);
    return hipGetLastError();
}
// workspace: tr_colred_workspace_bytes(M, 128)
hipError_t launch_tr_head2_dgrad_bnbwd(const float* dl, int64_t M, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step,
                                       float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda, const float* bz,
                                       int64_t ldbz, const float* bscale, const float* bshift, const float* bmu, const float* brstd,
                                       const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3, double* part,
                                       hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    hipLaunchKernelGGL(tr_head2_dgrad_sums_kernel, dim3(nb), dim3(256), 0, s, dl, M, drop_key(mult, ldm, p_drop), seed, step, W, ldw, da,
                       ldda, bz, ldbz, bscale, bshift, bmu, brstd, part);
    BnEpi e{};
    e.M = M, e.gamma = gamma, e.rstd = const_cast<float*>(brstd), e.dgamma = dgamma, e.dbeta = dbeta, e.k1 = k1, e.k2 = k2, e.k3 = k3;
    hipLaunchKernelGGL(tr_colred_final_kernel<2>, dim3((128 + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, nb, 128, nullptr, e);
    return hipGetLastError();
}
size_t tr_head2_wgrad_workspace_bytes(int64_t M) {
    return (size_t)((M + TR_RED_ROWS - 1) / TR_RED_ROWS) * H2_COLS * 2 * sizeof(double);
}
// sums (2 * H2_COLS float64): [0, 128) = dW[0][.], 128 / 129 = db[0] / db[1], [130, 258) = dW[1][.] (258, 259 unused)
hipError_t launch_tr_head2_wgrad(const float* dl, const float* z, int64_t M, int64_t ldz, const float* scale, const float* shift,
                                 int relu, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop,
                                 double* ws, float* dWb, hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    hipLaunchKernelGGL(tr_head2_wgrad_kernel, dim3(nb), dim3(256), 0, s, dl, z, M, ldz, scale, shift, relu, drop_key(mult, ldm, p_drop),
                       seed, step, ws);
    BnEpi e{};
    e.M = 2;                                                // layout code: head2
    e.mu = dWb;
    hipLaunchKernelGGL(tr_colred_final_kernel<3>, dim3((H2_COLS + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, ws, nb, H2_COLS, nullptr, e);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the first layer (c_in <= 8)
// conv1 of every stack takes 3, 4 or 8 input channels. Through the MFMA kernels that was a (M, 32) zero-padded copy of the
// points, a K = 32 linear whose weight is 90 % zeros, a statistics pass, and backward a 32 x 64 wgrad over the padded copy.
// Two VALU kernels instead (round 4):
//   forward  z[p][c] = b[c] + sum_k W[c][k] x[p][k] for the Mp rows of z (rows >= M see x = 0), with sum z, sum z^2 over the
//            M real rows taken in the same pass (float64 partials per 256 rows -> tr_colred_final_kernel<1>: the BatchNorm
//            epilogue of dal3_tr_bn_stats);
//   wgrad    dW[c][k] = sum_{p < M} dz[p][c] x[p][k]  (float64 partials per 256 rows, pairs of (c, k) entries as the two
//            sums of a "column": tr_colred_final_kernel<0> over c_out * KIN / 2 columns).
// Thread = 4 consecutive output channels (CO4 = c_out / 4 lanes per row) x 256 / CO4 row lanes; c_out = 64 or 128.
template <int KIN, int CO4>
__global__ __launch_bounds__(256) void tr_conv1_fwd_kernel(const float* __restrict__ x, int64_t M, int64_t Mp, int c_in, int64_t ldx,
                                                           const float* __restrict__ W, int64_t ldw, const float* __restrict__ bias,
                                                           float* __restrict__ z, int64_t ldz, double* __restrict__ part) {
    constexpr int C = 4 * CO4, RL = 256 / CO4;
    __shared__ double sm[2][RL][C];
    const int l = threadIdx.x % CO4, rl = threadIdx.x / CO4, c = 4 * l;
    float w[4][KIN];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < KIN; ++k) w[e][k] = k < c_in ? W[(int64_t)(c + e) * ldw + k] : 0.0f;
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + c);
    const int64_t r0 = (int64_t)blockIdx.x * TR_RED_ROWS, r1 = min(Mp, r0 + TR_RED_ROWS);
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    for (int64_t p = r0 + rl; p < r1; p += RL) {
        float xv[KIN];
#pragma unroll
        for (int k = 0; k < KIN; ++k) xv[k] = (k < c_in && p < M) ? x[p * ldx + k] : 0.0f;
        f32x4 o = b;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < KIN; ++k) o[e] = __builtin_fmaf(w[e][k], xv[k], o[e]);
        *reinterpret_cast<f32x4*>(z + p * ldz + c) = o;
        if (p < M) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s0[e] += o[e];
                s1[e] += (double)o[e] * o[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sm[0][rl][c + e] = s0[e];
        sm[1][rl][c + e] = s1[e];
    }
    __syncthreads();
    if (threadIdx.x < C) {
        double a0 = 0.0, a1 = 0.0;
        for (int i = 0; i < RL; ++i) {
            a0 += sm[0][i][threadIdx.x];
            a1 += sm[1][i][threadIdx.x];
        }
        const int64_t o = ((int64_t)blockIdx.x * C + threadIdx.x) * 2;
        part[o] = a0;
        part[o + 1] = a1;
    }
}
template <int KIN, int CO4>
__global__ __launch_bounds__(256) void tr_conv1_wgrad_kernel(const float* __restrict__ dz, int64_t lddz, const float* __restrict__ x,
                                                             int64_t M, int c_in, int64_t ldx, double* __restrict__ part) {
    constexpr int C = 4 * CO4, RL = 256 / CO4;
    extern __shared__ double c1_sm[];                       // [RL][C * KIN]
    const int l = threadIdx.x % CO4, rl = threadIdx.x / CO4, c = 4 * l;
    const int64_t r0 = (int64_t)blockIdx.x * TR_RED_ROWS, r1 = min(M, r0 + TR_RED_ROWS);
    double acc[4][KIN];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < KIN; ++k) acc[e][k] = 0.0;
    for (int64_t p = r0 + rl; p < r1; p += RL) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(dz + p * lddz + c);
        float xv[KIN];
#pragma unroll
        for (int k = 0; k < KIN; ++k) xv[k] = k < c_in ? x[p * ldx + k] : 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < KIN; ++k) acc[e][k] += (double)g[e] * (double)xv[k];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < KIN; ++k) c1_sm[(int64_t)rl * (C * KIN) + (c + e) * KIN + k] = acc[e][k];
    __syncthreads();
    for (int i = threadIdx.x; i < C * KIN; i += 256) {      // entry i = (channel, k): the row lanes in order
        double t = 0.0;
        for (int r = 0; r < RL; ++r) t += c1_sm[(int64_t)r * (C * KIN) + i];
        part[(int64_t)blockIdx.x * (C * KIN) + i] = t;       // = part[(blk * C' + i / 2) * 2 + i % 2], C' = C * KIN / 2
    }
}
bool tr_conv1_ok(int c_in, int c_out) { return c_in >= 1 && c_in <= 8 && (c_out == 64 || c_out == 128); }
size_t tr_conv1_workspace_bytes(int64_t Mp, int c_out) {     // forward: pairs per channel; wgrad: c_out * 8 entries per block
    return (size_t)((Mp + TR_RED_ROWS - 1) / TR_RED_ROWS) * c_out * 8 * sizeof(double);
}
hipError_t launch_tr_conv1_bn_stats(const float* x, int64_t M, int64_t Mp, int c_in, int64_t ldx, const float* W, int64_t ldw,
                                    const float* bias, int c_out, float* z, int64_t ldz, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                    float* scale, float* shift, double* part, hipStream_t s) {
    const int nb = (int)((Mp + TR_RED_ROWS - 1) / TR_RED_ROWS);
    const auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, s, x, M, Mp, c_in, ldx, W, ldw, bias, z, ldz, part);
    };
    if (c_in <= 4) {
        if (c_out == 64) go(tr_conv1_fwd_kernel<4, 16>); else go(tr_conv1_fwd_kernel<4, 32>);
    } else {
        if (c_out == 64) go(tr_conv1_fwd_kernel<8, 16>); else go(tr_conv1_fwd_kernel<8, 32>);
    }
    BnEpi e{};
    e.M = M, e.gamma = gamma, e.beta = beta, e.running_mean = running_mean, e.running_var = running_var;
    e.momentum = momentum, e.eps = eps, e.mu = mu, e.rstd = rstd, e.scale = scale, e.shift = shift;
    // (blocks of padding rows only write zero partials: harmless in the sums)
    hipLaunchKernelGGL(tr_colred_final_kernel<1>, dim3((c_out + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, nb, c_out, nullptr, e);
    return hipGetLastError();
}
// dW (c_out, c_in) float32, from 2 * C' float64 column sums with C' = c_out * KIN / 2 (KIN = 4 for c_in <= 4, else 8): entry i = c * KIN + k is sum (i % 2) of column i / 2
hipError_t launch_tr_conv1_wgrad(const float* dz, int64_t lddz, const float* x, int64_t M, int c_in, int64_t ldx, int c_out, double* part,
                                 float* dW, hipStream_t s) {
    const int nb = (int)((M + TR_RED_ROWS - 1) / TR_RED_ROWS);
    const int kin = c_in <= 4 ? 4 : 8, co4 = c_out / 4;
    const size_t lds = (size_t)(256 / co4) * c_out * kin * sizeof(double);
    const auto go = [&](auto kern) -> hipError_t {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), lds, s, dz, lddz, x, M, c_in, ldx, part);
        return hipSuccess;
    };
    hipError_t e;
    if (kin == 4)
        e = c_out == 64 ? go(tr_conv1_wgrad_kernel<4, 16>) : go(tr_conv1_wgrad_kernel<4, 32>);
    else
        e = c_out == 64 ? go(tr_conv1_wgrad_kernel<8, 16>) : go(tr_conv1_wgrad_kernel<8, 32>);
    if (e != hipSuccess) return e;
    const int Cp = c_out * kin / 2;
    BnEpi ep{};
    ep.M = 1 | ((int64_t)kin << 8) | ((int64_t)c_in << 16);  // layout code: conv1, kin columns computed per channel, c_in kept
    ep.mu = dW;
    hipLaunchKernelGGL(tr_colred_final_kernel<3>, dim3((Cp + TR_FIN_CH - 1) / TR_FIN_CH), dim3(256), 0, s, part, nb, Cp, nullptr, ep);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- max over points
// g[s][c] = max_p act(z[p][c]) over the `seg` points of segment s, with the index of the FIRST maximum for the
// backward pass. Block = 64 channels x 4 row-lanes over one of SEG_CHUNKS chunks of the segment; candidates meet
// through a 64-bit atomicMax over the keys of pool_key (dal3_device.h), under which the smallest index wins among
// equal values.
#define SEG_CHUNKS 16
__global__ __launch_bounds__(256) void tr_segmax_kernel(const float* __restrict__ z, int64_t ldz, int64_t seg, int C,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        unsigned long long* __restrict__ packed) {
    __shared__ unsigned long long sm[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int64_t s = blockIdx.y / SEG_CHUNKS;
    const int chunk = blockIdx.y % SEG_CHUNKS;
    const int64_t len = (seg + SEG_CHUNKS - 1) / SEG_CHUNKS;
    const int64_t p0 = chunk * len, p1 = min(seg, p0 + len);
    unsigned long long best = 0ull;
    if (c < C) {
        const float sc = scale[c], sh = shift[c];
        const float* zp = z + s * seg * ldz + c;
        float bv = -1.0f;
        int64_t bi = 0;
        for (int64_t p = p0 + rl; p < p1; p += 4) {
            const float y = fmaxf(zp[p * ldz] * sc + sh, 0.0f);
            if (y > bv) {
                bv = y;
                bi = p;
            }
        }
        if (bv >= 0.0f) best = pool_key(bv, (uint32_t)bi);
    }
    sm[rl][cl] = best;
    __syncthreads();
    if (rl == 0 && c < C) {
        unsigned long long b = sm[0][cl];
        for (int i = 1; i < 4; ++i) b = sm[i][cl] > b ? sm[i][cl] : b;
        atomicMax(packed + s * C + c, b);
    }
}

__global__ void tr_segmax_unpack_kernel(const unsigned long long* __restrict__ packed, int64_t n, float* __restrict__ g,
                                        int32_t* __restrict__ arg) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pool_unkey(packed[i], g[i], arg[i]);
}
hipError_t launch_tr_segmax_unpack(const unsigned long long* packed, int64_t total, float* g, int32_t* arg, hipStream_t s) {
    hipLaunchKernelGGL(tr_segmax_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, packed, total, g, arg);
    return hipGetLastError();
}

hipError_t launch_tr_segmax(const float* z, int64_t ldz, int64_t seg, int C, const float* scale, const float* shift,
                            float* g, int32_t* arg, int64_t n_seg, unsigned long long* packed, hipStream_t s) {
    hipError_t e = launch_fill_words(packed, (size_t)n_seg * C * 2, 0u, s);     // (a kernel: captured into hipGraphs, see dal3_misc.hip)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tr_segmax_kernel, dim3((C + 63) / 64, (unsigned)(n_seg * SEG_CHUNKS)), dim3(256), 0, s, z, ldz, seg, C,
                       scale, shift, packed);
    return launch_tr_segmax_unpack(packed, n_seg * C, g, arg, s);
}

// per-segment column sums: out[s][c] = sum_{p in segment s} x[p][c]  (gradient of the decoder's per-crop term).
// Block = 64 channels x 4 row-lanes over a whole segment; lane sums in double, added in lane order.
__global__ __launch_bounds__(256) void tr_segsum_kernel(const float* __restrict__ x, int64_t ldx, int64_t seg, int C,
                                                        float* __restrict__ out) {
    __shared__ double sm[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int64_t s = blockIdx.y;
    double acc = 0.0;
    if (c < C) {
        const float* xp = x + s * seg * ldx + c;
        double u0 = 0, u1 = 0, u2 = 0, u3 = 0;              // independent chains against the load latency
        int64_t p = rl;
        for (; p + 12 < seg; p += 16) {
            u0 += xp[p * ldx];
            u1 += xp[(p + 4) * ldx];
            u2 += xp[(p + 8) * ldx];
            u3 += xp[(p + 12) * ldx];
        }
        for (; p < seg; p += 4) u0 += xp[p * ldx];
        acc = (u0 + u1) + (u2 + u3);
    }
    sm[rl][cl] = acc;
    __syncthreads();
    if (rl == 0 && c < C) out[s * C + c] = (float)(((sm[0][cl] + sm[1][cl]) + sm[2][cl]) + sm[3][cl]);
}

hipError_t launch_tr_segsum(const float* x, int64_t ldx, int64_t seg, int C, float* out, int64_t n_seg, hipStream_t s) {
    hipLaunchKernelGGL(tr_segsum_kernel, dim3((C + 63) / 64, (unsigned)n_seg), dim3(256), 0, s, x, ldx, seg, C, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- segmentation loss
// The mask term of the three criteria (static_model.py:378-380, dynamic_model.py:337-339): mean over the M = B*N points
// of -log_softmax(logits)[label], two classes. One pass gives the per-point loss (reduced to one float64 per block, the
// blocks added in index order by a one-block second stage: reproducible) AND its gradient d loss_i / d logits_i =
// softmax - onehot, which the backward only has to scale by grad / M — instead of a label conversion, a log-softmax, an
// nll-loss and their three backward kernels over the same 2 MB (stock ops: 0.4 ms of a 11 ms step).
// labels: float32 (what the drivers' DataLoader delivers) or int64; values 0 / 1.
#define CE_BLOCK_PTS 2048
__global__ __launch_bounds__(256) void tr_seg_ce_kernel(const float* __restrict__ logits, const void* __restrict__ labels,
                                                        int labels_i64, int64_t M, float* __restrict__ dlogits,
                                                        double* __restrict__ part) {
    __shared__ double sm[4];
    const int64_t p0 = (int64_t)blockIdx.x * CE_BLOCK_PTS;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < CE_BLOCK_PTS / 256; ++u) {
        const int64_t p = p0 + u * 256 + threadIdx.x;
        if (p < M) {
            const f32x2 l = *reinterpret_cast<const f32x2*>(logits + 2 * p);
            const int y = labels_i64 ? (int)static_cast<const int64_t*>(labels)[p] : (int)static_cast<const float*>(labels)[p];
            const float mx = fmaxf(l[0], l[1]);
            const float e0 = expf(l[0] - mx), e1 = expf(l[1] - mx);
            const float sum = e0 + e1;
            const float lse = mx + logf(sum);
            acc += (double)(lse - (y ? l[1] : l[0]));
            f32x2 g;
            g[0] = e0 / sum - (y ? 0.0f : 1.0f);
            g[1] = e1 / sum - (y ? 1.0f : 0.0f);
            *reinterpret_cast<f32x2*>(dlogits + 2 * p) = g;
        }
    }
    // fixed-order block sum: lanes by xor butterfly (same pairs every run), the four waves in wave order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__global__ __launch_bounds__(256) void tr_seg_ce_final_kernel(const double* __restrict__ part, int n, int64_t M,
                                                              float* __restrict__ loss) {
    __shared__ double sm[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += part[i];
    sm[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += sm[i];
        *loss = (float)(t / (double)M);
    }
}

size_t tr_seg_ce_workspace_bytes(int64_t M) { return (size_t)((M + CE_BLOCK_PTS - 1) / CE_BLOCK_PTS) * sizeof(double); }

hipError_t launch_tr_seg_ce(const float* logits, const void* labels, int labels_i64, int64_t M, float* loss, float* dlogits,
                            double* part, hipStream_t s) {
    const int nb = (int)((M + CE_BLOCK_PTS - 1) / CE_BLOCK_PTS);
    hipLaunchKernelGGL(tr_seg_ce_kernel, dim3(nb), dim3(256), 0, s, logits, labels, labels_i64, M, dlogits, part);
    hipLaunchKernelGGL(tr_seg_ce_final_kernel, dim3(1), dim3(256), 0, s, part, nb, M, loss);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- box loss terms
// The five box terms of the criteria (static_model.py:382-424 per estimate, dynamic_model.py:341-383): centre (Huber of
// the L2 distance, delta 2), heading class (cross-entropy over 12 bins), heading residual (Huber, delta 1, of the
// predicted normalised residual of the LABEL's bin against label / (pi/12)), size class (cross-entropy over 3) and size
// residual (Huber, delta 1, of || label / mean_size[class] - predicted normalised residual of the label's class ||), each
// the mean over the B items — and the gradient of every mean w.r.t. its inputs, in the same pass. O(B) work that stock
// ops spread over ~60 launches per estimate and step. One workgroup; per-thread float64 sums over items tid, tid+256, ...,
// added in thread order (reproducible).
__constant__ float c_tr_mean_size[9] = {DAL3_MEAN_SIZE_VALUES};

struct BoxLossArgs {
    const float* center;        // (B,3)
    const float* center_label;  // (B,3)
    const float* hs;            // (B,12) heading scores
    const float* hrn;           // (B,12) normalised heading residuals
    const int64_t* hcl;         // (B,)
    const float* hrl;           // (B,)
    const float* ss;            // (B,3)  size scores
    const float* srn;           // (B,3,3) normalised size residuals
    const int64_t* scl;         // (B,)
    const float* srl;           // (B,3)
    float* losses;              // (5,): centre, heading class, heading residual, size class, size residual
    float* g_center;            // (B,3)   d losses[0] / d center
    float* g_hs;                // (B,12)  d losses[1] / d hs
    float* g_hrn;               // (B,12)  d losses[2] / d hrn
    float* g_ss;                // (B,3)   d losses[3] / d ss
    float* g_srn;               // (B,9)   d losses[4] / d srn
};

__global__ __launch_bounds__(256) void tr_box_loss_kernel(BoxLossArgs a, int B) {
    __shared__ double sm[5][256];
    const float inv_b = 1.0f / (float)B;
    double acc[5] = {0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < B; b += 256) {
        // centre
        float d[3], n2 = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d[k] = a.center[b * 3 + k] - a.center_label[b * 3 + k];
            n2 += d[k] * d[k];
        }
        const float dist = sqrtf(n2);
        float q = fminf(dist, 2.0f);
        acc[0] += (double)(0.5f * q * q + 2.0f * (dist - q));
#pragma unroll
        for (int k = 0; k < 3; ++k) a.g_center[b * 3 + k] = dist > 0.0f ? q * d[k] / dist * inv_b : 0.0f;
        // class labels out of range (an ignore value, a -1): F.nll_loss of the stock criterion raises; here every loss term
        // comes back NaN AND the item's gradient rows are NaN (round 4, ADVICE r3: with zeroed rows a loop that never looks
        // at the loss kept stepping the optimizer on a batch the reference would have rejected) — nothing is read out of bounds
        const int64_t hc64 = a.hcl[b], sc64 = a.scl[b];
        if (hc64 < 0 || hc64 >= 12 || sc64 < 0 || sc64 >= 3) {
            const float qn = __builtin_nanf("");
#pragma unroll
            for (int t = 0; t < 5; ++t) acc[t] = __builtin_nan("");
#pragma unroll
            for (int k = 0; k < 3; ++k) a.g_center[b * 3 + k] = a.g_ss[b * 3 + k] = qn;
#pragma unroll
            for (int k = 0; k < 12; ++k) a.g_hs[b * 12 + k] = a.g_hrn[b * 12 + k] = qn;
#pragma unroll
            for (int k = 0; k < 9; ++k) a.g_srn[b * 9 + k] = qn;
            continue;
        }
        // heading class
        const int hc = (int)hc64;
        float mx = a.hs[b * 12];
#pragma unroll
        for (int k = 1; k < 12; ++k) mx = fmaxf(mx, a.hs[b * 12 + k]);
        float e[12], sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            e[k] = expf(a.hs[b * 12 + k] - mx);
            sum += e[k];
        }
        acc[1] += (double)(mx + logf(sum) - a.hs[b * 12 + hc]);
#pragma unroll
        for (int k = 0; k < 12; ++k) a.g_hs[b * 12 + k] = (e[k] / sum - (k == hc ? 1.0f : 0.0f)) * inv_b;
        // heading residual of the label's bin
        const float er = a.hrn[b * 12 + hc] - a.hrl[b] / (float)(3.14159265358979323846 / 12.0);
        const float ae = fabsf(er);
        q = fminf(ae, 1.0f);
        acc[2] += (double)(0.5f * q * q + (ae - q));
#pragma unroll
        for (int k = 0; k < 12; ++k) a.g_hrn[b * 12 + k] = k == hc ? (er > 0.0f ? q : (er < 0.0f ? -q : 0.0f)) * inv_b : 0.0f;
        // size class
        const int sc = (int)sc64;
        const float s0 = a.ss[b * 3], s1 = a.ss[b * 3 + 1], s2 = a.ss[b * 3 + 2];
        const float smx = fmaxf(s0, fmaxf(s1, s2));
        const float f0 = expf(s0 - smx), f1 = expf(s1 - smx), f2 = expf(s2 - smx);
        const float fs = f0 + f1 + f2;
        acc[3] += (double)(smx + logf(fs) - a.ss[b * 3 + sc]);
        a.g_ss[b * 3 + 0] = (f0 / fs - (sc == 0 ? 1.0f : 0.0f)) * inv_b;
        a.g_ss[b * 3 + 1] = (f1 / fs - (sc == 1 ? 1.0f : 0.0f)) * inv_b;
        a.g_ss[b * 3 + 2] = (f2 / fs - (sc == 2 ? 1.0f : 0.0f)) * inv_b;
        // size residual of the label's class
        float v[3];
        n2 = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = a.srl[b * 3 + k] / c_tr_mean_size[sc * 3 + k] - a.srn[b * 9 + sc * 3 + k];
            n2 += v[k] * v[k];
        }
        const float sd = sqrtf(n2);
        q = fminf(sd, 1.0f);
        acc[4] += (double)(0.5f * q * q + (sd - q));
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int cls = k / 3, kk = k % 3;
            a.g_srn[b * 9 + k] = (cls == sc && sd > 0.0f) ? -q * v[kk] / sd * inv_b : 0.0f;
        }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) sm[t][threadIdx.x] = acc[t];
    __syncthreads();
    if (threadIdx.x < 5) {
        double s = 0.0;
        for (int i = 0; i < 256; ++i) s += sm[threadIdx.x][i];
        a.losses[threadIdx.x] = (float)(s / (double)B);
    }
}

hipError_t launch_tr_box_loss(const float* center, const float* center_label, const float* hs, const float* hrn,
                              const int64_t* hcl, const float* hrl, const float* ss, const float* srn, const int64_t* scl,
                              const float* srl, int B, float* losses, float* g_center, float* g_hs, float* g_hrn, float* g_ss,
                              float* g_srn, hipStream_t s) {
    BoxLossArgs a{center, center_label, hs, hrn, hcl, hrl, ss, srn, scl, srl, losses, g_center, g_hs, g_hrn, g_ss, g_srn};
    hipLaunchKernelGGL(tr_box_loss_kernel, dim3(1), dim3(256), 0, s, a, B);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- pooled layer, sparse terms
// The two B*C-sparse terms of the backward of  conv -> BN -> ReLU -> max over an item's points  (train.py
// _pooled_layer_backward): with row(b,c) = b*N + arg[b][c] the pooled point of channel c in item b and kd = k1 * dy there,
//     da[row(b,c)][:] += kd[b][c] * W[c][:]                  (scatter: several channels of an item can share a point)
//     dWs[c][:]        = sum_b kd[b][c] * a[row(b,c)][:]     (gather)
// Stock ops did the first as a 33 MB outer product + index_put_(accumulate=True) (a sort of the 65,536 row indices and two
// passes) and the second as a 33 MB gather + product + sum: 0.4 ms of a 9.6 ms step.
// Scatter, one workgroup per item, DETERMINISTIC without a global sort: the item's channels are bucketed by point in LDS
// (count, prefix sum, fill by atomic slot, then each point's short list is put in channel order), and each touched row is
// owned by one group of K/4 lanes that adds its channels' terms in that order and updates the row once.
// LDS: (2 N + C + 1) ints per item, at most 64 KiB (N = 5120 points and C = 1024 channels: 45 KiB).
// POOL_SLICES workgroups share an item: each buckets only the channels whose point falls into its slice of the point axis
// and owns those rows (one workgroup per item was a chain of dependent L2 / HBM round trips: 100-180 us).
#define POOL_SLICES 16
__global__ __launch_bounds__(256) void tr_pool_scatter_kernel(const int32_t* __restrict__ arg, const float* __restrict__ kd,
                                                              const float* __restrict__ W, int64_t ldw, int C, int K, int N,
                                                              float* __restrict__ da, int64_t ldda) {
    extern __shared__ int s_pool[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int per = (N + POOL_SLICES - 1) / POOL_SLICES;
    const int lo = blockIdx.y * per, hi = min(N, lo + per), n_loc = max(hi - lo, 0);   // this workgroup's points [lo, hi)
    const int C4 = (C + 3) & ~3;
    int* s_arg = s_pool;                                   // [C4] the item's pooled points (16-byte aligned: read as int4)
    int* list = s_pool + C4;                               // [C] channels grouped by point, in channel order
    int* pend = list + C;                                  // [C] the channels pooled inside [lo, hi), any order
    int* cnt = pend + C;                                   // [n_loc + 1] counts, then start offsets (exclusive prefix)
    int* fill = cnt + per + 1;                             // [n_loc] slots handed out
    __shared__ int s_part[256];
    __shared__ int s_nin;
    if (tid == 0) s_nin = 0;
    for (int p = tid; p <= n_loc; p += 256) cnt[p] = 0;
    for (int p = tid; p < n_loc; p += 256) fill[p] = 0;
    for (int c = tid; c < C; c += 256) s_arg[c] = arg[(int64_t)b * C + c];
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const int p = s_arg[c];
        if (p >= lo && p < hi) {
            atomicAdd(&cnt[p - lo], 1);
            pend[atomicAdd(&s_nin, 1)] = c;
        }
    }
    __syncthreads();
    // exclusive prefix sum over cnt[0..n_loc): a contiguous chunk per thread, then the 256 chunk totals
    const int chunk = (n_loc + 255) / 256, p0 = min(n_loc, tid * chunk), p1 = min(n_loc, p0 + chunk);
    int loc = 0;
    for (int p = p0; p < p1; ++p) loc += cnt[p];
    s_part[tid] = loc;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = s_part[i];
            s_part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    int run = s_part[tid];
    for (int p = p0; p < p1; ++p) {
        const int v = cnt[p];
        cnt[p] = run;
        run += v;
    }
    if (p1 == n_loc) cnt[n_loc] = run;                     // the total (every thread that gets here holds the same value)
    __syncthreads();
    // Channel order inside each point's list. Short lists (the usual case: a handful of channels per point): slots
    // handed out by an atomic counter, then an insertion sort by the point's thread. That is quadratic in the list's
    // length and run by ONE thread — with the tied maxima of zero-padded items (every channel of an item pooled at its
    // first point) it took 300 us of a DynamicModel step, 8 ms at worst — so the channels of LONG lists are placed by
    // rank instead: a channel's place = the number of lower channels pooled at the same point (a scan of the item's
    // points in LDS, eight 16-byte reads in flight), over the compacted list of this workgroup's channels so that only
    // as many waves scan as there are channels to place.
    constexpr int POOL_SORT_MAX = 12;
    const int n_in = s_nin;
    for (int t = tid; t < n_in; t += 256) {
        const int c = pend[t], p = s_arg[c] - lo;
        const int s0 = cnt[p], n = cnt[p + 1] - s0;
        if (n <= POOL_SORT_MAX) {
            list[s0 + atomicAdd(&fill[p], 1)] = c;
            continue;
        }
        const int pa = p + lo;
        int r = 0;
        const int4* v = reinterpret_cast<const int4*>(s_arg);
        const int n4 = c >> 2;
        int i = 0;
        for (; i + 8 <= n4; i += 8) {
            int4 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = v[i + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) r += (x[u].x == pa) + (x[u].y == pa) + (x[u].z == pa) + (x[u].w == pa);
        }
        for (int c2 = 4 * i; c2 < c; ++c2) r += s_arg[c2] == pa;
        list[s0 + r] = c;
    }
    __syncthreads();
    for (int p = tid; p < n_loc; p += 256) {
        const int s0 = cnt[p], n = cnt[p + 1] - s0;
        if (n > POOL_SORT_MAX) continue;
        for (int i = 1; i < n; ++i) {
            const int v = list[s0 + i];
            int j = i - 1;
            while (j >= 0 && list[s0 + j] > v) {
                list[s0 + j + 1] = list[s0 + j];
                --j;
            }
            list[s0 + j + 1] = v;
        }
    }
    __syncthreads();
    const int lanes = K / 4;                               // lanes per row: 16, 32 or 64
    const int grp = tid / lanes, n_grp = 256 / lanes, l = tid % lanes;
    for (int p = grp; p < n_loc; p += n_grp) {
        const int s0 = cnt[p], n = cnt[p + 1] - s0;
        if (n == 0) continue;
        f32x4* dst = reinterpret_cast<f32x4*>(da + ((int64_t)b * N + lo + p) * ldda + 4 * l);
        f32x4 o = *dst;                                    // (issued first: its latency passes under the channel loop)
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int i0 = 0; i0 < n; i0 += 4) {                // four channels' loads in flight, added in channel order
            float w[4];
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = list[s0 + min(i0 + u, n - 1)];
                w[u] = i0 + u < n ? kd[(int64_t)b * C + c] : 0.0f;
                v[u] = *reinterpret_cast<const f32x4*>(W + (int64_t)c * ldw + 4 * l);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[0] += w[u] * v[u][0];
                acc[1] += w[u] * v[u][1];
                acc[2] += w[u] * v[u][2];
                acc[3] += w[u] * v[u][3];
            }
        }
        o[0] += acc[0];
        o[1] += acc[1];
        o[2] += acc[2];
        o[3] += acc[3];
        *dst = o;
    }
}

// gather: one workgroup per channel, K threads x PG_L item lanes: lane l adds items l, l + L, ... in order (eight items'
// two-level loads — arg, then the row — in flight per trip), the lane sums are added in lane order: a fixed association.
// (Round 4: four lanes; one lane walked B = 64 items in eight trips of two dependent loads each: 23 us.)
#define PG_L 4
__global__ void tr_pool_gather_kernel(const int32_t* __restrict__ arg, const float* __restrict__ kd, const float* __restrict__ a,
                                      int64_t lda, int B, int C, int K, int N, float* __restrict__ dWs) {
    extern __shared__ float pg_sm[];                       // [PG_L][K]
    const int c = blockIdx.x, k = threadIdx.x % K, l = threadIdx.x / K;
    float acc = 0.0f;
    for (int b0 = l; b0 < B; b0 += 8 * PG_L) {
        float w[8], v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int bb = b0 + u * PG_L;
            const int b = min(bb, B - 1);
            const int64_t row = (int64_t)b * N + arg[(int64_t)b * C + c];
            w[u] = bb < B ? kd[(int64_t)b * C + c] : 0.0f;
            v[u] = a[row * lda + k];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += w[u] * v[u];
    }
    pg_sm[l * K + k] = acc;
    __syncthreads();
    if (l == 0) {
        float t = pg_sm[k];
#pragma unroll
        for (int j = 1; j < PG_L; ++j) t += pg_sm[j * K + k];
        dWs[(int64_t)c * K + k] = t;
    }
}

// zarg[b][c] = W[c] . a[b*N + arg[b][c]] + bias[c]: the pooled layer's PRE-BatchNorm value at each pooled point (what the
// backward's xhat needs; the fused forward never writes the layer's output). Sixteen lanes per (item, channel): each takes
// every 16th float4 of the two K-rows, partial dots in lane order through a fixed shuffle tree — deterministic. Replaces
// index arithmetic + a gather of B*C rows + a batched dot on stock ops (seven launches, 65 us at 64 x 1024 x 128).
__global__ __launch_bounds__(256) void tr_pool_zarg_kernel(const int32_t* __restrict__ arg, const float* __restrict__ a, int64_t lda,
                                                           const float* __restrict__ W, int64_t ldw, const float* __restrict__ bias,
                                                           int64_t n, int C, int K, int N, float* __restrict__ zarg) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    const int64_t ii = i < n ? i : n - 1;
    const int c = (int)(ii % C);
    const int64_t b = ii / C;
    const f32x4* ar = reinterpret_cast<const f32x4*>(a + (b * N + arg[ii]) * lda);
    const f32x4* wr = reinterpret_cast<const f32x4*>(W + (int64_t)c * ldw);
    float acc = 0.0f;
    for (int k = l; k < K / 4; k += 16) {
        const f32x4 x = ar[k], w = wr[k];
        acc += (x[0] * w[0] + x[1] * w[1]) + (x[2] * w[2] + x[3] * w[3]);
    }
    acc += __shfl_xor(acc, 8, 64);
    acc += __shfl_xor(acc, 4, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 1, 64);
    if (l == 0 && i < n) zarg[i] = acc + bias[c];
}
// out[s][c] = z[(s*seg + arg[s][c])][c]: the pre-BN value at each pooled point when the layer's output IS materialised
// (the point heads' unfused conv4 + max): one launch instead of the seven of a stock fancy-indexing expression
__global__ __launch_bounds__(256) void tr_gather_at_kernel(const float* __restrict__ z, int64_t ldz, const int32_t* __restrict__ arg,
                                                           int64_t seg, int64_t n, int C, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t s = i / C;
    const int c = (int)(i - s * C);
    out[i] = z[(s * seg + arg[i]) * ldz + c];
}
hipError_t launch_tr_gather_at(const float* z, int64_t ldz, const int32_t* arg, int64_t seg, int n_seg, int C, float* out, hipStream_t s) {
    const int64_t n = (int64_t)n_seg * C;
    hipLaunchKernelGGL(tr_gather_at_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, ldz, arg, seg, n, C, out);
    return hipGetLastError();
}

hipError_t launch_tr_pool_zarg(const int32_t* arg, const float* a, int64_t lda, const float* W, int64_t ldw, const float* bias, int B,
                               int C, int K, int N, float* zarg, hipStream_t s) {
    const int64_t n = (int64_t)B * C;
    hipLaunchKernelGGL(tr_pool_zarg_kernel, dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0, s, arg, a, lda, W, ldw, bias, n, C, K,
                       N, zarg);
    return hipGetLastError();
}

hipError_t launch_tr_pool_sparse(const int32_t* arg, const float* kd, const float* W, int64_t ldw, const float* a, int64_t lda,
                                 int B, int C, int K, int N, float* da, int64_t ldda, float* dWs, hipStream_t s) {
    const int per = (N + POOL_SLICES - 1) / POOL_SLICES;
    const size_t lds = (size_t)(2 * per + 1 + 3 * C + 4) * sizeof(int);
    hipLaunchKernelGGL(tr_pool_scatter_kernel, dim3(B, POOL_SLICES), dim3(256), lds, s, arg, kd, W, ldw, C, K, N, da, ldda);
    hipLaunchKernelGGL(tr_pool_gather_kernel, dim3(C), dim3(K * PG_L), (size_t)K * PG_L * sizeof(float), s, arg, kd, a, lda, B, C, K, N, dWs);
    return hipGetLastError();
}

// per-channel coefficients of the pooled layer's backward (train.py _pooled_layer_backward): D = dg * [g > 0] (the ReLU
// gate at the pooled point), xhat = (zarg - mu) * rstd,
//   dbeta = sum_b D, dgamma = sum_b D * xhat, k1 = gamma * rstd, k2 = dbeta / M, k3 = dgamma / M,
//   A = -k1 k2 + k1 k3 rstd mu, Bc = -k1 k3 rstd, kd[b][c] = k1 * D[b][c]            (float64 except kd)
// — two dozen stock launches on (C,) and (B, C) tensors otherwise. coef: (4, C) float64 = dbeta | dgamma | A | Bc.
// PC_CH channels x PC_L item lanes per workgroup: lane l adds items l, l + L, ... in order, the lane sums are added in
// lane order (deterministic; one thread per channel walking all B items was 74 us of dependent loads for B = 64).
#define PC_CH 16                         // channels per workgroup (round 4: 16 x 16 item lanes, was 64 x 4 — sixteen workgroups
#define PC_L 16                          // walking 16 items each in dependent trips: 24 us for a few hundred KB)
__global__ __launch_bounds__(256) void tr_pool_coef_kernel(const float* __restrict__ dg, const float* __restrict__ g,
                                                           const float* __restrict__ zarg, const float* __restrict__ mu,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           int B, int C, int64_t M, double* __restrict__ coef,
                                                           float* __restrict__ kd) {
    __shared__ double sm[2][PC_L][PC_CH];
    const int el = threadIdx.x % PC_CH, l = threadIdx.x / PC_CH;
    const int c = blockIdx.x * PC_CH + el;
    const bool live = c < C;
    const double m = live ? (double)mu[c] : 0.0, rs = live ? (double)rstd[c] : 0.0;
    double dbeta = 0.0, dgamma = 0.0;
    if (live) {
#pragma unroll 4
        for (int b = l; b < B; b += PC_L) {                 // lane l: items l, l + L, ... in order
            const int64_t i = (int64_t)b * C + c;
            const double D = g[i] > 0.0f ? (double)dg[i] : 0.0;
            dbeta += D;
            dgamma += D * (((double)zarg[i] - m) * rs);
        }
    }
    sm[0][l][el] = dbeta;
    sm[1][l][el] = dgamma;
    __syncthreads();
    if (!live) return;
    dbeta = dgamma = 0.0;
#pragma unroll
    for (int j = 0; j < PC_L; ++j) {                        // the lane sums in lane order: a fixed association
        dbeta += sm[0][j][el];
        dgamma += sm[1][j][el];
    }
    const double k1 = (double)gamma[c] * rs, k2 = dbeta / (double)M, k3 = dgamma / (double)M;
    if (l == 0) {
        coef[c] = dbeta;
        coef[C + c] = dgamma;
        coef[2 * C + c] = -k1 * k2 + k1 * k3 * rs * m;
        coef[3 * C + c] = -k1 * k3 * rs;
    }
#pragma unroll 4
    for (int b = l; b < B; b += PC_L) {
        const int64_t i = (int64_t)b * C + c;
        kd[i] = (float)(k1 * (g[i] > 0.0f ? (double)dg[i] : 0.0));
    }
}

hipError_t launch_tr_pool_coef(const float* dg, const float* g, const float* zarg, const float* mu, const float* rstd,
                               const float* gamma, int B, int C, int64_t M, double* coef, float* kd, hipStream_t s) {
    hipLaunchKernelGGL(tr_pool_coef_kernel, dim3((C + PC_CH - 1) / PC_CH), dim3(256), 0, s, dg, g, zarg, mu, rstd, gamma, B, C, M, coef,
                       kd);
    return hipGetLastError();
}

// ---- the float64 algebra of the pooled layer's shortcut (train.py _moments_through / _pooled_layer_backward) as three
// kernels instead of ~35 stock launches (W.double(), three rocBLAS dgemms of 16 MFLOP at 40 us each, products, sums,
// casts): K = the layer's input channels (64, 128 or 256: one thread per input channel), C its output channels (one
// workgroup each). All sums in float64 in a fixed order (loops in index order, LDS trees of a fixed shape).
// forward: [sum z, sum z^2] over the M points of z = W a + b from the moments of a: m1 = sum a (K), Sc = sum of the
// CENTRED a a^T (K x K, fp32 from the wgrad kernel):  mu_c = w_c . m1 / M + b_c,  var_c = max(w_c^T (Sc / M) w_c, 0),
// sums = [mu M | (var + mu^2) M]
__global__ __launch_bounds__(256) void tr_pool_moments_kernel(const float* __restrict__ W, int64_t ldw, const float* __restrict__ b,
                                                              const double* __restrict__ m1, const float* __restrict__ Sc,
                                                              int64_t M, int C, int K, double* __restrict__ sums) {
    __shared__ double wrow[256], red[256];
    const int c = blockIdx.x, k = threadIdx.x;
    wrow[k] = (double)W[(int64_t)c * ldw + k];
    __syncthreads();
    double t = 0.0;
#pragma unroll 8
    for (int j = 0; j < K; ++j) t += wrow[j] * (double)Sc[(int64_t)j * K + k];
    const double var = block_sum_f64(t * wrow[k] / (double)M, red, K);
    const double mean = block_sum_f64(wrow[k] * (m1[k] / (double)M), red, K);
    if (k == 0) {
        const double mu = mean + (double)b[c], v = var > 0.0 ? var : 0.0;
        sums[c] = mu * (double)M;
        sums[C + c] = (v + mu * mu) * (double)M;
    }
}

// backward, first half: G = W^T diag(Bc) W (K x K) and v = (A + Bc b)^T W (K), fp32 out (the operands of the linear
// kernel that forms da). coef = dbeta | dgamma | A | Bc (tr_pool_coef). The sums over the C channels are cut into
// TR_GV_SPLIT parts (one workgroup per row k1 of G — or v — and part; a whole sum per thread was 1,024 dependent trips,
// 51 us), float64 partials in ws, added in part order by the second kernel.
#define TR_GV_SPLIT 8
__global__ __launch_bounds__(256) void tr_pool_gv_kernel(const double* __restrict__ coef, const float* __restrict__ W, int64_t ldw,
                                                         const float* __restrict__ b, int C, int K, double* __restrict__ ws) {
    const int k1 = blockIdx.x, k2 = threadIdx.x, part = blockIdx.y;
    const int per = (C + TR_GV_SPLIT - 1) / TR_GV_SPLIT, c0 = part * per, c1 = min(C, c0 + per);
    const double* A = coef + 2 * (int64_t)C;
    const double* Bc = coef + 3 * (int64_t)C;
    double acc = 0.0;
    if (k1 < K) {
#pragma unroll 8
        for (int c = c0; c < c1; ++c) acc += Bc[c] * (double)W[(int64_t)c * ldw + k1] * (double)W[(int64_t)c * ldw + k2];
    } else {
#pragma unroll 8
        for (int c = c0; c < c1; ++c) acc += (A[c] + Bc[c] * (double)b[c]) * (double)W[(int64_t)c * ldw + k2];
    }
    ws[((int64_t)part * (K + 1) + k1) * K + k2] = acc;
}
__global__ __launch_bounds__(256) void tr_pool_gv_final_kernel(const double* __restrict__ ws, int K, float* __restrict__ G,
                                                               float* __restrict__ v) {
    const int k1 = blockIdx.x, k2 = threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int p = 0; p < TR_GV_SPLIT; ++p) acc += ws[((int64_t)p * (K + 1) + k1) * K + k2];
    if (k1 < K)
        G[(int64_t)k1 * K + k2] = (float)acc;
    else
        v[k2] = (float)acc;
}

// backward, second half: dW[c][k] = A_c m1_k + Bc_c ((W S)[c][k] + b_c m1_k) + dWs[c][k], with S = sum a a^T given either
// directly (centred == 0) or as the centred Sc + m1 m1^T / M (centred != 0); fp32 out
__global__ __launch_bounds__(256) void tr_pool_dw_kernel(const double* __restrict__ coef, const float* __restrict__ W, int64_t ldw,
                                                         const float* __restrict__ b, const float* __restrict__ S,
                                                         const double* __restrict__ m1, int64_t M, int centred,
                                                         const float* __restrict__ dWs, int C, int K, float* __restrict__ dW) {
    __shared__ double wrow[256], red[256];
    const int c = blockIdx.x, k = threadIdx.x;
    wrow[k] = (double)W[(int64_t)c * ldw + k];
    __syncthreads();
    double t = 0.0;
#pragma unroll 8
    for (int j = 0; j < K; ++j) t += wrow[j] * (double)S[(int64_t)j * K + k];
    const double m1k = m1[k];
    if (centred) t += block_sum_f64(wrow[k] * m1k, red, K) * m1k / (double)M;   // (W m1) m1^T / M
    const double A = coef[2 * (int64_t)C + c], Bc = coef[3 * (int64_t)C + c];
    dW[(int64_t)c * K + k] = (float)(A * m1k + Bc * (t + (double)b[c] * m1k) + (double)dWs[(int64_t)c * K + k]);
}

bool tr_pool_k_ok(int K) { return K == 64 || K == 128 || K == 256; }
hipError_t launch_tr_pool_moments(const float* W, int64_t ldw, const float* b, const double* m1, const float* Sc, int64_t M, int C,
                                  int K, double* sums, hipStream_t s) {
    if (!tr_pool_k_ok(K)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tr_pool_moments_kernel, dim3(C), dim3(K), 0, s, W, ldw, b, m1, Sc, M, C, K, sums);
    return hipGetLastError();
}
size_t tr_pool_gv_workspace_bytes(int K) { return (size_t)TR_GV_SPLIT * (K + 1) * K * sizeof(double); }
hipError_t launch_tr_pool_gv(const double* coef, const float* W, int64_t ldw, const float* b, int C, int K, float* G, float* v,
                             double* ws, hipStream_t s) {
    if (!tr_pool_k_ok(K)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tr_pool_gv_kernel, dim3(K + 1, TR_GV_SPLIT), dim3(K), 0, s, coef, W, ldw, b, C, K, ws);
    hipLaunchKernelGGL(tr_pool_gv_final_kernel, dim3(K + 1), dim3(K), 0, s, ws, K, G, v);
    return hipGetLastError();
}
hipError_t launch_tr_pool_dw(const double* coef, const float* W, int64_t ldw, const float* b, const float* S, const double* m1,
                             int64_t M, int centred, const float* dWs, int C, int K, float* dW, hipStream_t s) {
    if (!tr_pool_k_ok(K)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tr_pool_dw_kernel, dim3(C), dim3(K), 0, s, coef, W, ldw, b, S, m1, M, centred, dWs, C, K, dW);
    return hipGetLastError();
}

