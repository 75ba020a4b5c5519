// dal3_enc_screen.hip — the fp32 throughput encoder with conv5 SCREENED (DESIGN.md "Screened conv5").
//
// conv5 (128 -> 1024) is 89 % of the encoder's multiply-adds and the network keeps only the channel maxima of its
// output. Two launches replace ins_seg_encode_kernel<T> for large jobs; both run conv1..conv4 in fp32 exactly as the
// dense kernel does and then evaluate conv5 on the fp16 MFMA (16 x the fp32 rate) with a PROVED error bound
//   |s16(c,p) - chain32(c,p)| <= E_c = X * P_c + Q_c        (X >= ||x_p||_2 for every point of the wave),
// chain32 being the dense kernel's value (a k-ordered fmaf chain from a zero accumulator):
//   pass A  g[c] <- max(g[c], relu(fl(max_p s16 - E_c + b_c)))        a LOWER bound of the final value, in g itself;
//           the maximum over ANY subset of the crop's points is one, and pass A takes every DAL3_SCR_A_STRIDE-th
//           wave-slot of 64 points only (slot 0 always): a weaker threshold, more candidates, a fraction of the sweep
//   pass B  (c,p) is a candidate iff s16(c,p) > g[c] - b_c - E_c (rounded down); every candidate is recomputed with
//           the exact fp32 chain on the VALU (same operands, same order, same roundings as the f32 MFMA) and
//           relu(fl(chain + b_c)) goes to g with the same integer atomicMax as the dense kernel's.
// A pair that is not a candidate has fl(chain + b_c) <= g[c] already, so it cannot change g: the result has the dense
// kernel's bits. Whatever does not fit the proof or the lists takes the dense conv_max_layer, per wave: activations
// beyond fp16's range, conv5 weights beyond it (blob flag), more than SCR_CAP candidates in a 32-point tile.
// PASS B OWNS EVERY EXACT VALUE: it sweeps every point, and a wave that leaves the screen is computed densely there and
// nowhere else. Pass A only ever writes lower bounds from screened waves: a visited wave that leaves the screen
// contributes nothing, and with the blob's flag set pass A returns at once.
// Jobs with enough crops to fill the chip with whole-crop workgroups (enc_resident_route) take ONE launch instead,
// ins_seg_encode_resident_kernel: a workgroup owns a crop, its first round of slots is both pass A's subset and part of
// pass B, and every later slot is screened against the exact maxima of the slots before it. The sweep, the lists and the
// recompute are the same device code in all three kernels (scr_conv5_sweep, enc_screen_slot).
#include <cstddef>
#include "dal3_device.h"
#include "dal3_kernels.h"
#include "dal3_lp.h"
#include "dal3_screen.h"

#ifndef SCR_CAP
#define SCR_CAP 1024                    // candidate entries per wave and 32-point tile (bench input: 130 on average, 426 at most in the CPU model)
#endif
#define SCR_XLD 132                     // floats per point row of the LDS copy of x4: 128 + 4, rows start 4 banks apart
#define SCR_STAGE_LD 36                 // words per candidate row of the recompute's weight stage: a 32-channel slice + 4
#ifndef SCR_DEPTH
#define SCR_DEPTH 2                     // slices of the recompute in flight (measured 1 / 2 / 4: 4.13 / 4.12 / 4.19 ms, profiles/LEDGER_r13.md)
#endif
#define SCR_XMAX_BITS 0x476A6000        // 60000.0f: activations up to here round to a FINITE fp16
// Pass A visits the wave-slots (32 * DAL3_ENC_T consecutive points) of a crop whose index is a multiple of this stride.
// 1: every slot, the launches of the unstrided kernel (A/B builds). Measured (profiles/LEDGER_r13.md, lists built once
// per wave and staged recompute): the encoder at 4096 x 1024 takes 5.00 / 4.18 / 4.12 / 5.04 ms at 1 / 2 / 4 / 8 — 103 / 161
// candidates per 32-point tile at 2 / 4; at 8 pass B's candidates cost more than pass A still saves — and at 1024 x 5120
// 4.69 / 4.21 ms at 2 / 4, at 64 x 4096 0.252 / 0.234 ms.
#ifndef DAL3_SCR_A_STRIDE
#define DAL3_SCR_A_STRIDE 4
#endif
static_assert(DAL3_SCR_A_STRIDE >= 1, "pass A's stride over the wave-slots");

// Diagnostic build only (-DDAL3_SCREEN_COUNT): [0] waves, [1] waves dense for range, [2] waves dense for list overflow,
// [3] candidates, [4] recompute rounds. No counter executes in the shipped library.
#ifdef DAL3_SCREEN_COUNT
__device__ unsigned long long g_scr_count[8];
extern "C" int dal3_debug_screen_counts(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_scr_count), sizeof(g_scr_count));
    if (e == hipSuccess && reset) {
        unsigned long long z[8] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_scr_count), z, sizeof(z));
    }
    return (int)e;
}
#define SCR_COUNT(k, v)                                           \
    do {                                                          \
        if (lane == 0) atomicAdd(&g_scr_count[k], (unsigned long long)(v)); \
    } while (0)
#else
#define SCR_COUNT(k, v)
#endif

// The bound of the decoder's plan (DESIGN.md "Crop-dead channels of dconv1"), taken while conv2's output x2 is in
// registers: the wave's maximum over its points of dconv1a's fp16 score, per channel, into the workgroup's key table s_u
// (prune_key: the scores are signed), and X >= ||x2(p)||_2 of every point into s_x. The transposed orientation of the
// conv5 sweep: a lane is a channel, its registers are the points. A wave with an activation beyond fp16's range (or a
// blob whose dconv1a weights are beyond it) gives X = +Inf and no scores: its crop gets no plan.
// (Measured and not kept, profiles/LEDGER_r14.md: the epilogue cut into slices behind the next block's fragments with the
// ring started in front of conv2, and both lane halves sending their maxima without the exchange: each 0.08 ms slower.)
template <int T>
__device__ __forceinline__ void dec_prune_sweep(const InsSegW& w, const f32x16 (&x2)[T][2], uint32_t* s_u, int* s_x, int lane) {
    int xm = 0;
    float x2max = 0.0f;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        float ss = 0.0f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int v = __float_as_int(x2[j][kt][r]);         // >= +0 after the ReLU; a NaN pattern lies above the limit
                xm = v > xm ? v : xm;
                ss = fmaf(x2[j][kt][r], x2[j][kt][r], ss);
            }
        }
        ss += __shfl_xor(ss, 32);
        x2max = __builtin_fmaxf(x2max, ss);
    }
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) x2max = __builtin_fmaxf(x2max, __shfl_xor(x2max, d));
    const bool over = *w.prn_flag != 0 || __builtin_amdgcn_ballot_w64(xm > SCR_XMAX_BITS) != 0;
    const float X = sqrtf(x2max) * (1.0f + 0x1p-16f);              // (margin: 64 roundings of the sum, the root)
    if (lane == 0) atomicMax(s_x, over ? 0x7F800000 : __float_as_int(X));
    if (over) return;
    ActTile<FP16> xh[T][2];
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) xh[j][kt] = pack_relu<FP16>(x2[j][kt]);
    }
    WRing<4> r16;
    r16.init(w.w1h, lane);                             // [out-tile][kt][s]: a block's 4 fragments are fetched a block ahead
    f32x16 acc[2][T];
    auto fold = [&](const f32x16 (&a)[T], int mt) {    // the block's maxima -> the table
        float m = a[0][0];
#pragma unroll
        for (int j = 0; j < T; ++j) {
#pragma unroll
            for (int r = (j == 0 ? 1 : 0); r < 16; ++r) m = __builtin_fmaxf(m, a[j][r]);
        }
        m = __builtin_fmaxf(m, __shfl_xor(m, 32));
        if (lane < 32) atomicMax(&s_u[32 * mt + lane], prune_key(__float_as_uint(m)));
    };
#pragma unroll
    for (int mt = 0; mt < 16; ++mt) {
#pragma unroll
        for (int j = 0; j < T; ++j) acc[mt & 1][j] = f32x16{};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f16x8_t a = __builtin_bit_cast(f16x8_t, r16.slot[i]);
            r16.slot[i] = r16.fetch();
#pragma unroll
            for (int j = 0; j < T; ++j) acc[mt & 1][j] = FP16::mfma(xh[j][i >> 1].k[i & 1], a, acc[mt & 1][j]);
        }
        if (mt > 0) fold(acc[(mt - 1) & 1], mt - 1);   // (behind this block's MFMAs)
    }
    fold(acc[1], 15);
}

// The static LDS of a workgroup. CAND: the kernel takes candidates (pass B, the resident kernel) and holds the waves' x4
// copies, lists and stages; pass A needs the three tables only. One workgroup per CU by LDS alone (the kernels hold one
// wave per SIMD by registers anyway).
template <bool CAND, int T>
struct EncScreenLds {
    float b5[1024];                                    // conv5's folded bias
    int max[1024];                                     // the workgroup's maxima (bit patterns >= 0), as in the dense kernel
    f32x2 pq[1024];                                    // (P_c, Q_c)
    float g[CAND ? 1024 : 1];                          // the crop's row of g as the workgroup found it: thresholds
    float x[CAND ? DAL3_WG_WAVES * 32 * SCR_XLD : 4];  // the waves' x4 copies (16-byte rows: the asserts below)
    uint32_t list[CAND ? DAL3_WG_WAVES * T * SCR_CAP : 1];
    // per wave: the sweep's parked hit words (32 blocks x 64 lanes), then the recompute's staged weight rows
    uint32_t stage[CAND ? DAL3_WG_WAVES * 64 * SCR_STAGE_LD : 4];
    uint32_t u[CAND ? 512 : 1];                        // with `prune`: the workgroup's keys of dconv1a's score maxima
    int xn[1];                                         // ... and the bits of its X
};
using EncScreenLdsB = EncScreenLds<true, DAL3_ENC_T>;
static_assert(offsetof(EncScreenLdsB, x) % 16 == 0 && offsetof(EncScreenLdsB, stage) % 16 == 0,
              "x and stage are read and written 16 bytes at a time (the struct itself is placed on 16 bytes)");
// Too large: lower SCR_CAP, DAL3_WG_WAVES or DAL3_ENC_T.
static_assert(22 * 1024 + 64 + DAL3_WG_WAVES * (32 * SCR_XLD * 4 + DAL3_ENC_T * SCR_CAP * 4 + 64 * SCR_STAGE_LD * 4) <= 160 * 1024 &&
                  sizeof(EncScreenLds<true, DAL3_ENC_T>) <= 22 * 1024 + 64 + DAL3_WG_WAVES * (32 * SCR_XLD * 4 + DAL3_ENC_T * SCR_CAP * 4 + 64 * SCR_STAGE_LD * 4),
              "pass B's and the resident kernel's LDS exceeds a CU's 160 KiB: lower SCR_CAP, DAL3_WG_WAVES or DAL3_ENC_T");
static_assert(32 * 64 <= 64 * SCR_STAGE_LD, "a wave's stage holds the hit words of conv5's 32 blocks");

// conv5's fp16 sweep over a wave's T tiles, the one piece of code of every kernel below. PASS 0: the bound phase, the
// maxima of the scores minus E into L.max; PASS 1: the candidate phase, one hit word per block parked in `stage`.
// RISING (the resident kernel): the threshold is the larger of the crop's row of g and the workgroup's own table AS IT
// STANDS when the block's constant is taken — whatever another wave has added by then is <= the final value, which is
// all the proof asks of G. The compare is an integer one on the bit patterns (L.max >= 0 always; a non-finite pattern of
// either table lies above every finite value and is final for its channel), so no NaN pattern is ever read as a value.
template <int PASS, bool RISING, int T, class Lds>
__device__ __forceinline__ void scr_conv5_sweep(const InsSegW& w, const ActTile<FP16> (&xh)[T][4], float X, Lds& L, uint32_t* stage,
                                                ScreenHits<T>& hits, int lane) {
    // Per 32-channel block the wave holds ONE constant per lane (= channel): pass A the error bound E_c, pass B the
    // threshold on the fp16 score. chain32 <= s16 + E; s16 <= thr <= G - b - E  ==>  chain32 + b <= G  ==>
    // fl(chain32 + b) <= G: such a pair cannot raise g. (E, thr: every rounding is covered by the 2^-20 / 2^-22 terms.)
    auto block_const = [&](int mt) -> float {
        const int c = 32 * mt + (lane & 31);
        const f32x2 pq = L.pq[c];
        float E = fmaf(X, pq[0], pq[1]);
        E = fmaf(E, 0x1p-20f, E);
        if (PASS == 0) return E;
        float G = L.g[c];
        const float bb = L.b5[c];
        if (RISING) {
            const int own = L.max[c], row = __float_as_int(G);
            G = __int_as_float(own > row ? own : row);
        }
        if (bits_nonfinite(G)) return 3.0e38f;         // above every finite score: no candidate (decided on the bit pattern)
        return (G - bb) - fmaf(__builtin_fabsf(G) + __builtin_fabsf(bb), 0x1p-22f, E);
    };
    // The epilogue of a block is cut into 8 slices (registers 2i, 2i+1 of every tile) that ride behind the MFMAs
    // of the NEXT block's fragment i, like MaxEpilogueT's steps: pass A a running max, pass B one bit per
    // (tile, register) whose score is above the threshold (scr_push_hit: 32 pushes replace the whole word). The
    // block's word is parked and counted; the lists are built once, after the sweep (dal3_screen.h).
    static_assert(16 * T <= 32, "one hit bit per (tile, register) in a 32-bit word");
    float m = 0.0f;
    uint32_t hb = 0;
    auto ep_slice = [&](const f32x16 (&acc)[T], int i, float k) {
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const int r = 2 * i + rr;
                if (PASS == 0)
                    m = (r == 0 && j == 0) ? acc[0][0] : __builtin_fmaxf(m, acc[j][r]);
                else
                    hb = scr_push_hit(hb, acc[j][r], k);
            }
        }
    };
    auto ep_finish = [&](int mt, float k) {
        const int c = 32 * mt + (lane & 31);
        if (PASS == 0) {
            m = __builtin_fmaxf(m, __shfl_xor(m, 32));
            // y <= max_p chain32 (the subtraction's own rounding is inside the 2^-22 term); x -> fl(x + b) is monotone
            const float y = m - fmaf(__builtin_fabsf(m), 0x1p-22f, k);
            int bits = __float_as_int(y + L.b5[c]);
            bits = bits > 0 ? bits : 0;
            if (lane < 32 && bits > 0) atomicMax(&L.max[c], bits);
        } else {
            hits.park_block(stage, mt, hb, lane);
        }
    };

    WRing<8> r16;
    r16.init(w.w5h, lane);                             // [out-tile][kt][s] fragments of 1 KiB; a block's 8 are fetched a block ahead
    // transposed tile, as conv_max_layer: points on the registers, channels on the lanes
    auto mm = [&](f32x16 (&acc)[T], auto side) {
#pragma unroll
        for (int j = 0; j < T; ++j) acc[j] = f32x16{};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f16x8_t a = __builtin_bit_cast(f16x8_t, r16.slot[i]);
            r16.slot[i] = r16.fetch();
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = FP16::mfma(xh[j][i >> 1].k[i & 1], a, acc[j]);
            DAL3_SCHED_FENCE();
            side(i);
            DAL3_SCHED_FENCE();
        }
    };
    f32x16 accA[T], accB[T];
    float kA = block_const(0), kB;
    mm(accA, NoSide());                                                    // block 0
    int mt = 1;
    for (; mt + 1 < 32; mt += 2) {                     // (two whole blocks per trip and nothing else: see conv_max_layer)
        kB = block_const(mt);
        mm(accB, [&](int i) { ep_slice(accA, i, kA); });
        ep_finish(mt - 1, kA);
        kA = block_const(mt + 1);
        mm(accA, [&](int i) { ep_slice(accB, i, kB); });
        ep_finish(mt, kB);
    }
    kB = block_const(mt);                                                  // mt == 31
    mm(accB, [&](int i) { ep_slice(accA, i, kA); });
    ep_finish(mt - 1, kA);
#pragma unroll
    for (int i = 0; i < 8; ++i) ep_slice(accB, i, kB);                     // last block: nothing left to hide under
    ep_finish(mt, kB);
}

// One wave-slot (32 T consecutive points from n0 of crop b) through conv1..conv4 and the screened conv5.
//   MODE 0  pass A: the bound phase alone
//   MODE 1  pass B: the candidate phase (sweep, lists, exact recompute), or the dense layer for a wave that leaves the screen
//   MODE 2  the resident kernel: pass B's body on the rising table; `first` (round 0, uniform in the workgroup): the bound
//           phase on the same x4 / xh, then ONE workgroup barrier, then the candidate phase. Every wave of the workgroup
//           meets that barrier: an idle one (n0 beyond the crop) and a dense one as well, which contribute no bound.
template <int MODE, int T, class Lds>
__device__ __forceinline__ void enc_screen_slot(const InsSegW& w, BCN pts, int c_in, int n_pts, int64_t b, int n0, bool with_prune,
                                                bool first, Lds& L, int lane, int wave) {
    const int h = lane >> 5;
    const bool active = n0 < n_pts;                    // (no early return: every wave meets the barriers)
    f32x16 x4[T][4];
    WRing<DAL3_PF> ring;
    bool dense = false;
    if (active) {
        ring.init(w.enc_stream, lane);                 // conv2 | conv3 | conv4 | conv5
        f32x16 bias = tile_from_channels(w.b2, h);
        float in[T][2];
        load_points<2, T>(pts, b, n0, n_pts, c_in, in, lane);
        f32x16 x1[T][2], x2[T][2], x3[T][2];
        first_layer<2, 2, T>(w.w1, w.b1, in, x1, lane);
        mlp_layer_ring<2, 2, T>(ring, w.b2, w.b3, bias, x1, x2, lane);
        if (MODE != 0 && with_prune) dec_prune_sweep<T>(w, x2, L.u, L.xn, lane);
        mlp_layer_ring<2, 2, T>(ring, w.b3, w.b4, bias, x2, x3, lane);
        mlp_layer_ring<2, 4, T>(ring, w.b4, w.b4, bias, x3, x4, lane);
        SCR_COUNT(0, 1);

        // fp16 holds every activation of the wave? (x4 >= +0 after the ReLU: the integer order of the bit patterns is
        // the order of the values, and a NaN / Inf pattern lies above the limit.) The decision depends on the wave's
        // own points and the blob only; it matters where exact values are owed, which see every wave.
        int xm = 0;
#pragma unroll
        for (int j = 0; j < T; ++j) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int v = __float_as_int(x4[j][kt][r]);
                    xm = v > xm ? v : xm;
                }
            }
        }
        // conv5 not finite in fp16 (the blob's flag): no wave can be screened
        dense = *w.scr_flag != 0 || __builtin_amdgcn_ballot_w64(xm > SCR_XMAX_BITS) != 0;
        if (dense) {
            // the bound phase has nothing for this wave; the candidate phase computes its exact values
            SCR_COUNT(1, 1);
            if (MODE == 1) conv_max_layer<4, T>(ring, L.b5, x4, reinterpret_cast<float*>(L.max), 32, lane);
        }
    }
    const bool screened = active && !dense;
    float X = 0.0f;
    ActTile<FP16> xh[T][4];
    if (screened) {
        // X >= ||x_p||_2 for every point of the wave (lane half h holds 64 of a point's 128 channels)
        float x2max = 0.0f;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            float ss = 0.0f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ss = fmaf(x4[j][kt][r], x4[j][kt][r], ss);
            }
            ss += __shfl_xor(ss, 32);
            x2max = __builtin_fmaxf(x2max, ss);
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) x2max = __builtin_fmaxf(x2max, __shfl_xor(x2max, d));
        X = sqrtf(x2max) * (1.0f + 0x1p-16f);          // (margin: 128 roundings of the sum, the root, the products below)
#pragma unroll
        for (int j = 0; j < T; ++j) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) xh[j][kt] = pack_relu<FP16>(x4[j][kt]);
        }
    }
    uint32_t* const list = L.list + (MODE != 0 ? wave * T * SCR_CAP : 0);
    uint32_t* const stage = L.stage + (MODE != 0 ? wave * 64 * SCR_STAGE_LD : 0);
    ScreenHits<T> hits;
    hits.init();
    if (MODE == 2) {
        if (first) {
            if (screened) scr_conv5_sweep<0, false, T>(w, xh, X, L, stage, hits, lane);
            __syncthreads();
        }
        if (active && dense) {                         // (the first stream's ring is not kept across the bound phase)
            WRing<DAL3_PF> r32;
            r32.init(w.enc_stream + ENC_W5 * 64, lane);
            conv_max_layer<4, T>(r32, L.b5, x4, reinterpret_cast<float*>(L.max), 32, lane);
        }
    }
    if (screened) {
        scr_conv5_sweep<(MODE == 0 ? 0 : 1), MODE == 2, T>(w, xh, X, L, stage, hits, lane);
        if (MODE != 0) {
            uint32_t cnt[T];
            const bool overflow = scr_build_lists<T, 32, SCR_CAP>(stage, list, hits, cnt, lane);
#pragma unroll
            for (int j = 0; j < T; ++j) SCR_COUNT(3, cnt[j]);
            if (overflow) {                            // the lists do not hold the tile's candidates: the dense layer, exact
                SCR_COUNT(2, 1);
                WRing<DAL3_PF> r32;
                r32.init(w.enc_stream + ENC_W5 * 64, lane);
                conv_max_layer<4, T>(r32, L.b5, x4, reinterpret_cast<float*>(L.max), 32, lane);
            } else {
                float* const xw = L.x + wave * 32 * SCR_XLD;
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    // this tile's x4 in fp32, point-major, channels in natural order: registers 4q..4q+3 of k-tile
                    // kt are channels 32kt + 8q + 4h .. +3 of point lane&31
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            f32x4 v;
                            v[0] = x4[j][kt][4 * q + 0];
                            v[1] = x4[j][kt][4 * q + 1];
                            v[2] = x4[j][kt][4 * q + 2];
                            v[3] = x4[j][kt][4 * q + 3];
                            *reinterpret_cast<f32x4*>(xw + (lane & 31) * SCR_XLD + 32 * kt + 8 * q + 4 * h) = v;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    // one candidate per lane: the dense kernel's chain from +0 (scr_recompute)
                    SCR_COUNT(4, (cnt[j] + 63) / 64);
                    scr_recompute<32, 4, SCR_DEPTH, true>(
                        w.w5row, 128, list + j * SCR_CAP, cnt[j], xw, SCR_XLD, stage, lane, [](uint32_t, bool) { return 0.0f; },
                        [&](float a, int c, uint32_t, bool live) {
                            int bits = __float_as_int(a + L.b5[c]);
                            bits = bits > 0 ? bits : 0;
                            if (live && bits > 0) atomicMax(&L.max[c], bits);
                        });
                }
            }
        }
    }
}

// The tables of a workgroup, and its maxima to g (and the prune row) at its end: one global atomic per positive channel.
// No early exit for a crop flagged by nonfinite_rows_kernel: its quiet-NaN pattern lies above every value any kernel here
// sends to atomicMax, exactly as for the dense kernel. A non-finite threshold (that pattern, or +Inf / NaN written by
// a dense wave of a crop whose activations overflow fp32) is final for its channel: no candidate is taken there.
template <bool CAND, int T>
__device__ __forceinline__ void enc_screen_tables(const InsSegW& w, EncScreenLds<CAND, T>& L, int* gi) {
    for (int i = threadIdx.x; i < 1024; i += 64 * DAL3_WG_WAVES) {
        L.b5[i] = w.b5[i];
        L.max[i] = 0;
        L.pq[i] = reinterpret_cast<const f32x2*>(w.scr_pq)[i];
        // (other workgroups of the crop may be raising g already: any value read here is <= the final one, which is all
        // the threshold needs)
        if (CAND) L.g[i] = __int_as_float(__hip_atomic_load(gi + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (CAND && i < 512) L.u[i] = 0;
    }
    if (threadIdx.x == 0) L.xn[0] = 0;
    __syncthreads();
}
template <bool CAND, int T>
__device__ __forceinline__ void enc_screen_flush(EncScreenLds<CAND, T>& L, int* gi, uint32_t* pu) {
    __syncthreads();
    for (int c = threadIdx.x; c < 1024; c += 64 * DAL3_WG_WAVES) {
        const int v = L.max[c];
        if (v > 0) atomicMax(gi + c, v);
    }
    if (CAND && pu) {                                  // one global atomic per channel and workgroup, as for g
        for (int c = threadIdx.x; c < 512; c += 64 * DAL3_WG_WAVES) {
            const uint32_t v = L.u[c];
            if (v > 0) atomicMax(pu + c, v);
        }
        if (threadIdx.x == 0 && L.xn[0] > 0) atomicMax(reinterpret_cast<int*>(pu + 512), L.xn[0]);
    }
}

// The two launches: a workgroup's four waves take four consecutive slots of one crop (pass A: four consecutive VISITED ones).
template <int PASS, int T>
__global__ __launch_bounds__(64 * DAL3_WG_WAVES) void ins_seg_encode_screen_kernel(InsSegW w, BCN pts, int c_in, int n_pts,
                                                                                  int tiles_per_item, float* __restrict__ g,
                                                                                  uint32_t* __restrict__ prune) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x / tiles_per_item;
    const int n0 = ((blockIdx.x % tiles_per_item) * DAL3_WG_WAVES + wave) * (PASS == 0 ? DAL3_SCR_A_STRIDE : 1) * (32 * T);
    __shared__ __attribute__((aligned(16))) EncScreenLds<PASS == 1, T> L;
    int* gi = reinterpret_cast<int*>(g + b * 1024);
    // conv5 not finite in fp16 (the blob's flag): pass A has no bound to give and pass B is the dense encoder. (Uniform: one word.)
    if (PASS == 0 && *w.scr_flag != 0) return;
    enc_screen_tables(w, L, gi);
    enc_screen_slot<PASS, T>(w, pts, c_in, n_pts, b, n0, prune != nullptr, false, L, lane, wave);
    enc_screen_flush(L, gi, PASS == 1 && prune ? prune + b * 513 : nullptr);
}

// The resident kernel: ONE workgroup owns a crop (blockIdx.x) and takes its slots in R = ceil(slots / 4) rounds, wave w
// slot r + R w of round r: round 0 visits slots 0, R, 2R, 3R — a strided subset like pass A's, slot 0 always in it — and
// gives the bound; every later slot is screened against the bound AND the exact maxima of the slots before it, which
// the workgroup holds in its own table (DESIGN.md "Screened conv5", the resident route). conv1..conv4 run once per
// point, the tables are loaded once per crop, and g / prune take one flush per crop. Rounds need no barrier between them.
template <int T>
__global__ __launch_bounds__(64 * DAL3_WG_WAVES) void ins_seg_encode_resident_kernel(InsSegW w, BCN pts, int c_in, int n_pts,
                                                                                    float* __restrict__ g, uint32_t* __restrict__ prune) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    __shared__ __attribute__((aligned(16))) EncScreenLds<true, T> L;
    int* gi = reinterpret_cast<int*>(g + b * 1024);
    enc_screen_tables(w, L, gi);
    const int slots = (n_pts + 32 * T - 1) / (32 * T);
    const int R = (slots + DAL3_WG_WAVES - 1) / DAL3_WG_WAVES;
    for (int r = 0; r < R; ++r)
        enc_screen_slot<2, T>(w, pts, c_in, n_pts, b, (r + R * wave) * (32 * T), prune != nullptr, r == 0, L, lane, wave);
    enc_screen_flush(L, gi, prune ? prune + b * 513 : nullptr);
}

hipError_t launch_ins_seg_encode_screen(const InsSegW& w, BCN pts, int c_in, int B, int N, float* g, hipStream_t s, uint32_t* prune) {
    constexpr int T = DAL3_ENC_T;
    const dim3 block(64 * DAL3_WG_WAVES);
    if (enc_resident_route(pts.flags, B, N)) {
        hipLaunchKernelGGL((ins_seg_encode_resident_kernel<T>), dim3((unsigned)B), block, 0, s, w, pts, c_in, N, g, prune);
        return hipGetLastError();
    }
    const int tpi = (N + 32 * DAL3_WG_WAVES * T - 1) / (32 * DAL3_WG_WAVES * T);
    // pass A: ceil(slots / stride) visited wave-slots per crop, DAL3_WG_WAVES of them per workgroup
    const int slots = (N + 32 * T - 1) / (32 * T);
    const int tpi_a = ((slots + DAL3_SCR_A_STRIDE - 1) / DAL3_SCR_A_STRIDE + DAL3_WG_WAVES - 1) / DAL3_WG_WAVES;
    const dim3 grid_a((unsigned)((int64_t)B * tpi_a)), grid((unsigned)((int64_t)B * tpi));
    hipLaunchKernelGGL((ins_seg_encode_screen_kernel<0, T>), grid_a, block, 0, s, w, pts, c_in, N, tpi_a, g, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ins_seg_encode_screen_kernel<1, T>), grid, block, 0, s, w, pts, c_in, N, tpi, g, prune);
    return hipGetLastError();
}
