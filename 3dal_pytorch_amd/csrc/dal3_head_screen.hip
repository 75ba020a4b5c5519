// dal3_head_screen.hip — the fp32 point heads with conv4 SCREENED (DESIGN.md "Screened conv4 of the point heads").
//
// The box head is conv1..conv4 (3 -> 128 -> 128 -> 256 -> 512) and a max over the item's object points; conv4 is 73 %
// of the multiply-adds and only its 512 channel maxima are kept. Jobs with enough items to fill the chip with whole-item
// workgroups (head_resident_route) take ONE launch, point_head_resident_kernel, described below; other large jobs are
// two launches over two worklists (nonfinite_rows_kernel, dal3_misc.hip):
//   seed launch      point_head_pers_kernel, UNCHANGED and dense, over each item's SEED tiles (the live tiles whose index
//                    is a multiple of DAL3_HEAD_SCR_STRIDE; tile 0 always): exact values in `feat`;
//   screened launch  this kernel over the other live tiles: conv1..conv3 in fp32 exactly as the dense kernel does, conv4
//                    on the fp16 MFMA with the encoder's proved bound restated for K = 256,
//                        |s16(c,p) - chain32(c,p)| <= E_c = X * P_c + Q_c     (X >= ||x_p||_2 for every point of the tile),
//                    (c,p) is a candidate iff s16 > thr = fl(fl(G - b_c) - fl(E + 2^-22 (|G| + |b_c|))); every candidate is
//                    recomputed with the exact k-ordered fmaf chain on the VALU, then + b, ReLU on the bits, into the
//                    run's LDS row, which is flushed to `feat` as the dense kernel's is.
// G is any value that is <= the final feat[item][c]: the seed's exact maximum as read when the run enters the item
// (possibly raised by other waves already), and the run's own exact maxima so far. A pair that is not a candidate has
// fl(chain + b_c) <= G, so it cannot change the result: the bits are the dense kernel's. The two launches have no
// lower-bound pass: conv1..conv3 are 27 % of the head, and a pass of its own that recomputes them costs more than it saves.
// Whatever does not fit the proof or the list takes the dense conv_max_layer, per tile: activations beyond fp16's range,
// conv4 weights beyond it (blob flag), more than HEAD_SCR_CAP candidates in the tile.
//   resident launch  one workgroup of DAL3_WG_WAVES waves owns an item at a time (one workgroup per CU, items from a
//                    cursor) and takes its live tiles in R = ceil(tiles / waves) rounds, wave w tile r + R w of
//                    round r. NO tile is dense for being a seed: in round 0 every wave
//                    first sweeps its tile in BOUND mode — per channel relu(fl(max_p s16 - E + b)), a lower bound of the
//                    final value, into the workgroup's ONE table of 512 patterns (loaded from the item's row of feat:
//                    0, or the quiet-NaN pattern) — then, after the workgroup's only barrier, screens the same x3 / xh
//                    registers against the table; conv1..conv3 run once per point. Later rounds screen against the
//                    table as it stands, raised by every exact value so far. All the proof asks of the table is
//                    G <= the final value (the resident route). The tile's body — range test, X, pack, sweep,
//                    lists, two-half recompute, dense fall-back — is the same device code in both kernels
//                    (head_conv4_sweep, head_screen_tile).
#include <cstddef>
#include "dal3_device.h"
#include "dal3_kernels.h"
#include "dal3_lp.h"
#include "dal3_screen.h"

#ifndef HEAD_SCR_CAP
#define HEAD_SCR_CAP 1024               // candidate entries per 32-point tile (CPU model, bench crops: at most 856 at stride 4)
#endif
#define HEAD_SCR_XLD 132                // floats per point row of the LDS copy of HALF of x3: 128 + 4, rows start 4 banks apart
#define HEAD_SCR_SW 16                  // channels per slice of the recompute's weight stage (rows of 16 + 4 words: what the CU's LDS leaves)
#ifndef HEAD_RES_SW
#define HEAD_RES_SW 32                  // ... of the resident kernel, whose tables are shared by four waves: rows of 32 + 4 fit its LDS
#endif                                  // (its four waves reach the recompute together; measured 16 / 32: profiles/LEDGER_r18.md)
#ifndef HEAD_SCR_DEPTH
#define HEAD_SCR_DEPTH 1                // slices in flight, of the 8 of a half of k: a second one already spills (x3 alone is 128 registers)
#endif
#define HEAD_SCR_XMAX_BITS 0x476A6000   // 60000.0f: activations up to here round to a FINITE fp16
#ifndef HEAD_RUN
#define HEAD_RUN 6                      // as point_head_pers_kernel
#endif

// Diagnostic build only (-DDAL3_SCREEN_COUNT): [0] tiles, [1] tiles dense for range or flag, [2] tiles dense for list
// overflow, [3] candidates, [4] recompute rounds (64 candidates, both halves of k); the resident kernel also [8 + r]
// candidates and [40 + r] screened tiles of round r (31: that round and every later one). No counter executes in the
// shipped library.
#ifdef DAL3_SCREEN_COUNT
#define HEAD_SCR_COUNTS 72
__device__ unsigned long long g_head_scr_count[HEAD_SCR_COUNTS];
extern "C" int dal3_debug_head_screen_counts(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_head_scr_count), sizeof(g_head_scr_count));
    if (e == hipSuccess && reset) {
        unsigned long long z[HEAD_SCR_COUNTS] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_head_scr_count), z, sizeof(z));
    }
    return (int)e;
}
#define HSCR_COUNT(k, v)                                                    \
    do {                                                                    \
        if (lane == 0) atomicAdd(&g_head_scr_count[k], (unsigned long long)(v)); \
    } while (0)
#else
#define HSCR_COUNT(k, v)
#endif

// Diagnostic build only (-DDAL3_STAMP, tools/stamps_head.py): a persistent wave sums the s_memtime ticks of its tiles' phases
// and leaves them, 16 words per wave, in a buffer of their own (dal3_debug_set_head_stamps): [0] conv1..conv3 with the next
// tile's entry and points, [1] norm, pack and range test, [2] the fp16 sweep, [3] list building, [4] / [5] the recompute's
// halves, [6] flush, entry and turnover, [7] a dense conv4 (range, flag or overflow), [8] tiles, [9] tiles that stayed
// screened; the resident kernel (a wave of a workgroup, 4 blockIdx.x + wave): [10] round 0's bound sweep, [11] the wait at
// its barrier. No stamp executes in the shipped library.
#ifdef DAL3_STAMP
struct HeadStamps {
    uint32_t acc[12];
    unsigned long long prev;
};
__device__ unsigned long long* g_head_stamps = nullptr;
extern "C" int dal3_debug_set_head_stamps(void* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_head_stamps), &p, sizeof(p));
}
#define HSTAMP_NOW(t)                                                               \
    do {                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                          \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                          \
    } while (0)
#define HSTAMP(k)                                \
    do {                                         \
        unsigned long long t_;                   \
        HSTAMP_NOW(t_);                          \
        st.acc[k] += (uint32_t)(t_ - st.prev);   \
        st.prev = t_;                            \
    } while (0)
#define HSTAMP_ADD(k, v) st.acc[k] += (v)
#else
struct HeadStamps {};
#define HSTAMP(k)
#define HSTAMP_ADD(k, v)
#endif

// The static LDS of a workgroup of WAVES waves: the tables once, then per wave the list, the partial chains, HALF of x3
// (a whole point-major x3 is 33 KiB per wave and does not fit) and the stage. The two launches run four one-wave
// workgroups per CU (one wave per SIMD at this register count), the resident kernel one workgroup of four waves: either
// way a CU's 160 KiB must hold it.
template <int WAVES, int SW_ = HEAD_SCR_SW>
struct HeadScreenLds {
    static constexpr int SW = SW_;
    f32x2 pq[512];                                     // (P_c, Q_c)
    float b4[512];                                     // conv4's folded bias
    int tab[512];                                      // the item's channel maxima (bit patterns; >= 0, or the quiet-NaN row's)
    uint32_t list[WAVES * HEAD_SCR_CAP];               // a tile's candidates: channel << 8 | point
    float part[WAVES * HEAD_SCR_CAP];                  // their chains after the first half of k
    float x[WAVES * 32 * HEAD_SCR_XLD];                // half of x3, point-major
    // per wave: the sweep's parked hit words (16 blocks x 64 lanes), then the recompute's staged weight rows
    uint32_t stage[WAVES * 64 * (SW_ + 4)];
    int g[WAVES == 1 ? 512 : 4];                       // the two launches: feat[item] as read when the run entered the item
};
using HeadResLds = HeadScreenLds<DAL3_WG_WAVES, HEAD_RES_SW>;
static_assert(offsetof(HeadScreenLds<1>, x) % 16 == 0 && offsetof(HeadScreenLds<1>, stage) % 16 == 0 &&
                  offsetof(HeadResLds, x) % 16 == 0 && offsetof(HeadResLds, stage) % 16 == 0 &&
                  (32 * HEAD_SCR_XLD * 4) % 16 == 0 && (64 * (HEAD_SCR_SW + 4) * 4) % 16 == 0 && (64 * (HEAD_RES_SW + 4) * 4) % 16 == 0,
              "x and stage are read and written 16 bytes at a time (the struct itself is placed on 16 bytes)");
static_assert(4 * sizeof(HeadScreenLds<1>) <= 160 * 1024 && sizeof(HeadResLds) <= 160 * 1024 && DAL3_WG_WAVES == 4,
              "the screened head's LDS exceeds a CU's 160 KiB: lower HEAD_SCR_CAP, HEAD_SCR_XLD or HEAD_SCR_SW");
static_assert(16 * 64 <= 64 * (HEAD_SCR_SW + 4) && 16 * 64 <= 64 * (HEAD_RES_SW + 4), "the stage holds the hit words of conv4's 16 blocks");

// conv4's fp16 sweep over one tile, the one piece of code of both kernels. PASS 0: the bound phase (resident kernel, round 0):
// per channel the maximum score of the tile, minus E, plus b, ReLU, into L.tab; PASS 1: the candidate phase, one hit
// word per block parked in `stage`. OWN_G (the two launches): the threshold is the larger of L.g and L.tab; otherwise L.tab
// alone, AS IT STANDS when the block's constant is taken — whatever another wave has added by then is <= the final value,
// which is all the proof asks of G. The compare is an integer one on the bit patterns (a non-finite pattern lies above
// every finite value and is final for its channel), so no NaN pattern is ever read as a value.
// The sweep consumes conv4's fp16 stream [16 out-tiles][8 kt][2 s] of 1 KiB exactly, so the ring stands at the stream's
// start (fragments 0..7 in the slots) at every tile boundary, whichever way the tile went and however many sweeps it
// ran, and the fetch behind use i of block mt is fragment (16 mt + i + 8) mod 256: a function of the counters, nothing
// carried round the tile loop. (A carried offset meets the dense routes' epilogue at the loop's join, a divergent
// branch the compiler merges from both routes, is taken for divergent there, and every fetch of the sweep gets a
// waterfall loop: profiles/LEDGER_r17.md.)
template <int PASS, bool OWN_G, class Lds>
__device__ __forceinline__ void head_conv4_sweep(WRing<8>& r16, const ActTile<FP16> (&xh)[8], float X, uint32_t vmask, Lds& L,
                                                 uint32_t* stage, ScreenHits<1>& hits, int lane) {
    constexpr int KT = 8;
    // Per 32-channel block one constant per lane (= channel): the bound phase's E, or the threshold on the fp16 score.
    // chain32 <= s16 + E; s16 <= thr <= G - b - E  ==>  chain32 + b <= G  ==>  fl(chain32 + b) <= G.
    auto block_const = [&](int mt) -> float {
        const int c = 32 * mt + (lane & 31);
        const f32x2 pq = L.pq[c];
        float E = fmaf(X, pq[0], pq[1]);
        E = fmaf(E, 0x1p-20f, E);
        if (PASS == 0) return E;
        int gb = L.tab[c];                                         // exact values (or lower bounds) of this item, patterns >= 0
        if (OWN_G) {
            const int gs = L.g[c];
            gb = gs > gb ? gs : gb;
        }
        const float G = __int_as_float(gb), bb = L.b4[c];
        if (bits_nonfinite(G)) return 3.0e38f;                     // above every finite score: no candidate (decided on the bit pattern)
        return (G - bb) - fmaf(__builtin_fabsf(G) + __builtin_fabsf(bb), 0x1p-22f, E);
    };
    // candidate phase: one hit bit per accumulator register (= point), collected in 8 slices behind the NEXT block's
    // first MFMAs; the block's word is parked and counted, the list is built once after the sweep (dal3_screen.h).
    // bound phase: a running maximum in the same slices. (The ragged last tile's copies of the item's last point are
    // in it: a copy's score IS that point's, the same operands through the same MFMA, so the maximum is unchanged.)
    uint32_t hb = 0;
    float m = 0.0f;
    auto ep_slice = [&](const f32x16& acc, int i, float k) {
        if (PASS == 0) {
            m = i == 0 ? __builtin_fmaxf(acc[0], acc[1]) : __builtin_fmaxf(__builtin_fmaxf(m, acc[2 * i]), acc[2 * i + 1]);
        } else {
            hb = scr_push_hit(hb, acc[2 * i], k);
            hb = scr_push_hit(hb, acc[2 * i + 1], k);
        }
    };
    auto ep_finish = [&](int mt, float k) {
        if (PASS == 0) {
            const int c = 32 * mt + (lane & 31);
            m = __builtin_fmaxf(m, __shfl_xor(m, 32));
            // y <= max_p chain32 (the subtraction's own rounding is inside the 2^-22 term); x -> fl(x + b) is monotone
            const float y = m - fmaf(__builtin_fabsf(m), 0x1p-22f, k);
            int bits = __float_as_int(y + L.b4[c]);
            bits = bits > 0 ? bits : 0;
            if (lane < 32 && bits > 0) atomicMax(&L.tab[c], bits);
        } else {
            hits.park_block(stage, mt, hb & vmask, lane);
        }
    };
    // transposed tile, as conv_max_layer: points on the registers, channels on the lanes
    auto mm = [&](f32x16& acc, int mt, auto side) {
        acc = f32x16{};
#pragma unroll
        for (int i = 0; i < 2 * KT; ++i) {
            const f16x8_t a = __builtin_bit_cast(f16x8_t, r16.slot[i & 7]);
            r16.slot[i & 7] = r16.fetch_at(((16u * (uint32_t)mt + (uint32_t)i + 8u) & 255u) * 1024u);
            acc = FP16::mfma(xh[i >> 1].k[i & 1], a, acc);
            DAL3_SCHED_FENCE();
            side(i);
            DAL3_SCHED_FENCE();
        }
    };
    f32x16 accA, accB;
    float kA = block_const(0), kB;
    mm(accA, 0, NoSide());                                                 // block 0
    int mt = 1;
    for (; mt + 1 < 16; mt += 2) {             // (two whole blocks per trip and nothing else: see conv_max_layer)
        kB = block_const(mt);
        mm(accB, mt, [&](int i) { if (i < 8) ep_slice(accA, i, kA); });
        ep_finish(mt - 1, kA);
        kA = block_const(mt + 1);
        mm(accA, mt + 1, [&](int i) { if (i < 8) ep_slice(accB, i, kB); });
        ep_finish(mt, kB);
    }
    kB = block_const(mt);                                                  // mt == 15
    mm(accB, mt, [&](int i) { if (i < 8) ep_slice(accA, i, kA); });
    ep_finish(mt - 1, kA);
#pragma unroll
    for (int i = 0; i < 8; ++i) ep_slice(accB, i, kB);                     // last block: nothing left to hide under
    ep_finish(mt, kB);
}

// One tile from conv3's output x3 (tile e_t of an item of e_n distinct points) through the screened conv4, into L.tab.
//   RES false  the two launches' screened body
//   RES true   the resident kernel: `first` (round 0, uniform in the workgroup): the bound phase on x3 / xh, then ONE
//              workgroup barrier, then the candidate phase on the same registers. Every wave of the workgroup meets that
//              barrier: an idle one (!active) and one that leaves the screen as well, which contribute no bound.
// w4f32: conv4's fp32 fragments on the head's stream, for the dense conv_max_layer of a tile that leaves the screen.
template <bool RES, class Lds>
__device__ __forceinline__ void head_screen_tile(const PointHeadW& w, const f32x4* w4f32, WRing<8>& r16, const f32x16 (&x3)[1][8],
                                                 int e_t, int e_n, bool blob_dense, bool active, bool first, int round, Lds& L,
                                                 int wave, int lane, HeadStamps& st) {
    constexpr int T = 1, KT = 8;
    const int h = lane >> 5;
    uint32_t* const s_list = L.list + wave * HEAD_SCR_CAP;
    float* const s_part = L.part + wave * HEAD_SCR_CAP;
    float* const s_x = L.x + wave * 32 * HEAD_SCR_XLD;
    uint32_t* const s_stage = L.stage + wave * 64 * (Lds::SW + 4);
    auto dense_tile = [&]() {                          // the dense kernel's conv4 + max on this tile, from a ring of its own
        WRing<DAL3_PF> r32;
        r32.init(w4f32, lane);
        conv_max_layer<KT, T>(r32, L.b4, x3, reinterpret_cast<float*>(L.tab), 16, lane);
    };
    // fp16 holds every activation of the tile? (x3 >= +0 after the ReLU: the integer order of the bit patterns is the
    // order of the values, and a NaN / Inf pattern lies above the limit.)
    bool dense = false;
    if (active) {
        int xm = 0;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int v = __float_as_int(x3[0][kt][r]);
                xm = v > xm ? v : xm;
            }
        }
        dense = blob_dense || __builtin_amdgcn_ballot_w64(xm > HEAD_SCR_XMAX_BITS) != 0;
    }
    const bool screened = active && !dense;
    float X = 0.0f;
    ActTile<FP16> xh[KT];
    uint32_t vmask = 0;
    if (screened) {
        // X >= ||x_p||_2 for every point of the tile (lane half h holds 128 of a point's 256 channels)
        float ss = 0.0f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) ss = fmaf(x3[0][kt][r], x3[0][kt][r], ss);
        }
        ss += __shfl_xor(ss, 32);
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) ss = __builtin_fmaxf(ss, __shfl_xor(ss, d));
        X = sqrtf(ss) * (1.0f + 0x1p-15f);             // (margin: 256 roundings of the sum, the root, the products below)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) xh[kt] = pack_relu<FP16>(x3[0][kt]);
        // the ragged last tile of an item repeats the item's last point (load_points): a copy is never listed, the
        // point itself is in this tile. vmask: accumulator register r of this lane half is a point of its own, at
        // the bit scr_push_hit leaves it (15 - r).
        const int left = e_n - e_t * 32;                                 // >= 1
#pragma unroll
        for (int r = 0; r < 16; ++r) vmask |= tile_chan(r, h) < left ? (1u << (15 - r)) : 0u;
        HSTAMP(1);
    }
    ScreenHits<T> hits;
    hits.init();
    if (RES && first) {
        if (screened) head_conv4_sweep<0, false>(r16, xh, X, vmask, L, s_stage, hits, lane);
        HSTAMP(10);
        __syncthreads();
        HSTAMP(11);
    }
    if (active && dense) {
        HSCR_COUNT(1, 1);
        dense_tile();
        HSTAMP(7);
    }
    if (screened) {
        head_conv4_sweep<1, !RES>(r16, xh, X, vmask, L, s_stage, hits, lane);
        HSTAMP(2);
        uint32_t cnt1[T];
        const bool overflow = scr_build_lists<T, 16, HEAD_SCR_CAP>(s_stage, s_list, hits, cnt1, lane);
        const uint32_t cnt = cnt1[0];
        HSCR_COUNT(3, cnt);
        if (RES) {
            HSCR_COUNT(8 + (round < 31 ? round : 31), cnt);
            HSCR_COUNT(40 + (round < 31 ? round : 31), 1);
        }
        HSTAMP(3);

        if (overflow) {                                // the list does not hold the tile's candidates: the dense layer, exact
            HSCR_COUNT(2, 1);
            dense_tile();
            HSTAMP(7);
        } else {
            // One candidate per lane: the dense kernel's chain. v_mfma_f32_32x32x2_f32 from a zero accumulator is, per
            // output, fma(a1, b1, fma(a0, b0, acc)) over its k-steps in issue order, k = 0 from lane half 0: channels
            // 8i, 8i+4, 8i+1, 8i+5, ... for i = 4 kt + q. The operands are staged in TWO HALVES of k (channels
            // 0..127, then 128..255); the chain crosses the halves through s_part, its order unchanged.
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                // this half of x3 in fp32, point-major, channels in natural order: registers 4q..4q+3 of k-tile kt
                // are channels 32kt + 8q + 4h .. +3 of point lane&31
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4 v;
                        v[0] = x3[0][4 * half + kt][4 * q + 0];
                        v[1] = x3[0][4 * half + kt][4 * q + 1];
                        v[2] = x3[0][4 * half + kt][4 * q + 2];
                        v[3] = x3[0][4 * half + kt][4 * q + 3];
                        *reinterpret_cast<f32x4*>(s_x + (lane & 31) * HEAD_SCR_XLD + 32 * kt + 8 * q + 4 * h) = v;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (half == 1) HSCR_COUNT(4, (cnt + 63) / 64);
                scr_recompute<Lds::SW, 128 / Lds::SW, HEAD_SCR_DEPTH, false>(
                    w.w4row + 128 * half, 256, s_list, cnt, s_x, HEAD_SCR_XLD, s_stage, lane,
                    [&](uint32_t idx, bool live) { return half == 0 ? 0.0f : s_part[live ? idx : 0u]; },
                    [&](float a, int c, uint32_t idx, bool live) {
                        if (half == 0) {
                            if (live) s_part[idx] = a;
                        } else {
                            int bits = __float_as_int(a + L.b4[c]);
                            bits = bits > 0 ? bits : 0;
                            if (live && bits > 0) atomicMax(&L.tab[c], bits);
                        }
                    });
                HSTAMP(4 + half);
            }
            HSTAMP_ADD(9, 1u);
        }
    }
}

template <int KS, int C1, int C2, int C3>
__global__ __launch_bounds__(64) void point_head_screen_kernel(PointHeadW w, BCN x, int c_in, float* __restrict__ feat,
                                                               uint32_t* __restrict__ ctl, const u32x4* __restrict__ list) {
    constexpr int T = 1;
    constexpr int KT = C3 / 32;                        // k-tiles of conv4
    static_assert(C3 == 256, "the bound, the two halves of k and the fp16 fragments are laid out for conv4 256 -> 512");
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    __shared__ __attribute__((aligned(16))) HeadScreenLds<1> L;        // tab: the current item's maxima of this run
    for (int i = threadIdx.x; i < 512; i += 64) {
        L.b4[i] = w.b4[i];
        L.tab[i] = 0;
        L.pq[i] = reinterpret_cast<const f32x2*>(w.scr_pq)[i];
    }
    __syncthreads();
    const uint32_t n_live = ctl[0];
    uint32_t run0 = n_live / (2u * gridDim.x);         // the guided schedule of point_head_pers_kernel
    run0 = run0 < 1u ? 1u : (run0 > HEAD_RUN ? HEAD_RUN : run0);
    const uint32_t first_free = gridDim.x * run0;
    uint32_t cur = blockIdx.x * run0, run_end = cur + run0;
    if (cur >= n_live) return;
    const bool blob_dense = *w.scr_flag != 0;          // a folded conv4 weight is not finite in fp16: every tile is dense

    constexpr uint32_t FRAGS23 = ((C2 / 32) * (C1 / 32) + (C3 / 32) * (C2 / 32)) * 4u;   // conv2 | conv3 fragments
    WRing<DAL3_PF, true> ring;                         // conv2 | conv3, cyclic: conv4's fp32 fragments are the fallback's
    ring.init(w.stream, lane, FRAGS23 * 1024u);
    WRing<8> r16;                                      // conv4's fp16 fragments (head_conv4_sweep)
    r16.init(w.w4h, lane);
    f32x16 bias = tile_from_channels(w.b2, h);
    u32x4 e = list[cur];
    float in[T][KS];
    load_points<KS, T>(x, (int64_t)e[0], (int)e[1] * 32, (int)e[2], c_in, in, lane);
    auto enter = [&](int64_t b) {                      // the item's thresholds (other waves may be raising them: any value read is <= the final one)
        const int* gi = reinterpret_cast<const int*>(feat + b * 512);
#pragma unroll
        for (int c = lane; c < 512; c += 64) L.g[c] = __hip_atomic_load(gi + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto flush = [&](int64_t b) {                      // the finished item's maxima -> feat (nothing where the value is 0)
        int* gi = reinterpret_cast<int*>(feat + b * 512);
#pragma unroll
        for (int c = lane; c < 512; c += 64) {
            const int v = L.tab[c];
            if (v > 0) atomicMax(gi + c, v);
            L.tab[c] = 0;
        }
    };
    enter((int64_t)e[0]);
    HeadStamps st;
#ifdef DAL3_STAMP
    st = HeadStamps{};
    HSTAMP_NOW(st.prev);
#endif
    for (;;) {
        const int64_t b = (int64_t)e[0];
        const int e_t = (int)e[1], e_n = (int)e[2];    // this tile's index and the item's distinct points
        const bool last_of_run = cur + 1 >= run_end || cur + 1 >= n_live;
        uint32_t nxt = 0, take = 1;
        if (last_of_run) {
            const uint32_t left = n_live > run_end ? n_live - run_end : 0u;
            take = left / (2u * gridDim.x);
            take = take < 1u ? 1u : (take > HEAD_RUN ? HEAD_RUN : take);
            if (lane == 0) nxt = atomicAdd(&ctl[1], take);
        }
        f32x16 x3[T][KT];
        float in_n[T][KS];
        uint32_t ncur, nend;
        {
            f32x16 x1[T][C1 / 32], x2[T][C2 / 32];
            first_layer<KS, C1 / 32, T>(w.w1, w.b1, in, x1, lane);
            mlp_layer_ring<C1 / 32, C2 / 32, T>(ring, w.b2, w.b3, bias, x1, x2, lane);
            if (last_of_run) {
                ncur = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt) + first_free;
                nend = ncur + take;
            } else {
                ncur = cur + 1;
                nend = run_end;
            }
            const uint32_t nclamp = ncur < n_live ? ncur : cur;
            e = list[nclamp];
            mlp_layer_ring<C2 / 32, C3 / 32, T>(ring, w.b3, w.b2, bias, x2, x3, lane);   // leaves bias = conv2's tile 0
            load_points<KS, T>(x, (int64_t)e[0], (int)e[1] * 32, (int)e[2], c_in, in_n, lane);
        }
        HSCR_COUNT(0, 1);
        HSTAMP(0);
        HSTAMP_ADD(8, 1u);
        head_screen_tile<false>(w, w.stream + FRAGS23 * 64, r16, x3, e_t, e_n, blob_dense, true, false, 0, L, 0, lane, st);
        const bool more = ncur < n_live;
        const bool leave = !more || (int64_t)e[0] != b;
        if (leave) flush(b);                           // (the wave's own LDS operations are in order: no barrier)
        HSTAMP(6);
        if (!more) break;
        if (leave) enter((int64_t)e[0]);
        HSTAMP(6);
        cur = ncur;
        run_end = nend;
#pragma unroll
        for (int k = 0; k < KS; ++k) in[0][k] = in_n[0][k];
    }
#ifdef DAL3_STAMP
    if (lane == 0 && blockIdx.x < 1024) {
#pragma unroll
        for (int k = 0; k < 10; ++k) g_head_stamps[blockIdx.x * 16 + k] = st.acc[k];
    }
#endif
}

// The resident kernel: a workgroup OWNS an item at a time, reads its count of distinct points itself (the clamp of
// nonfinite_rows_kernel's worklist) and takes its live tiles in R = ceil(tiles / waves) rounds, wave w tile r + R w of
// round r: round 0 visits tiles 0, R, 2R, 3R — a strided subset like the two launches' seeds, tile 0 always in it — and
// gives the bound; every later tile is screened against the bound AND the exact maxima of the tiles before it, which the
// workgroup holds in its one table. The table is loaded once per item and feat takes one flush per item: the row is this
// workgroup's alone (0 or the quiet-NaN pattern as nonfinite_rows_kernel left it, same stream), so the flush is a plain
// store of the table. Rounds need no barrier between them.
// The grid is one workgroup per CU (the LDS holds one), and a workgroup takes item blockIdx.x, then items from `cursor`
// (one word, zeroed on the stream before the launch): the bias, the bound's coefficients and both weight rings are set up
// once per workgroup, not per item. With one workgroup per item instead, every item paid a workgroup's launch and set-up
// with the CU otherwise empty, and a batch a little above a whole number of items per CU an extra, nearly empty round: at
// 4096 x 512 that grid took 2.94 ms against this one's 2.43 and the two launches' 2.76 (profiles/LEDGER_r18.md).
template <int KS, int C1, int C2, int C3>
__global__ __launch_bounds__(64 * DAL3_WG_WAVES) void point_head_resident_kernel(PointHeadW w, BCN x, int c_in, int n_pts,
                                                                                float* __restrict__ feat,
                                                                                const int32_t* __restrict__ distinct, int B,
                                                                                uint32_t* __restrict__ cursor) {
    constexpr int T = 1;
    constexpr int KT = C3 / 32;
    static_assert(C3 == 256, "the bound, the two halves of k and the fp16 fragments are laid out for conv4 256 -> 512");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int h = lane >> 5;
    __shared__ __attribute__((aligned(16))) HeadResLds L;
    __shared__ int s_item;
    for (int i = threadIdx.x; i < 512; i += 64 * DAL3_WG_WAVES) {
        L.b4[i] = w.b4[i];
        L.pq[i] = reinterpret_cast<const f32x2*>(w.scr_pq)[i];
    }
    const bool blob_dense = *w.scr_flag != 0;          // a folded conv4 weight is not finite in fp16: every tile is dense
    constexpr uint32_t FRAGS23 = ((C2 / 32) * (C1 / 32) + (C3 / 32) * (C2 / 32)) * 4u;   // conv2 | conv3 fragments
    WRing<DAL3_PF, true> ring;                         // conv2 | conv3, cyclic, as in the two launches
    ring.init(w.stream, lane, FRAGS23 * 1024u);
    WRing<8> r16;
    r16.init(w.w4h, lane);
    f32x16 bias = tile_from_channels(w.b2, h);
    HeadStamps st;
#ifdef DAL3_STAMP
    st = HeadStamps{};
    HSTAMP_NOW(st.prev);
#endif
    for (int64_t b = blockIdx.x;;) {                   // (gridDim.x <= B: the first item exists)
        int* const gi = reinterpret_cast<int*>(feat + b * 512);
        // (the thread's index is made opaque per use: hoisted out of the item loop, its 64-bit row address is one more
        // live register pair than the kernel has, and spills)
        int i0 = threadIdx.x;
        asm volatile("" : "+v"(i0));
        for (int i = i0; i < 512; i += 64 * DAL3_WG_WAVES) L.tab[i] = gi[i];
        __syncthreads();                               // (the first item's also covers b4 and pq)
        int n_eff = n_pts;
        if (distinct) {
            const int d = distinct[b];
            n_eff = d <= 0 ? 1 : (d < n_pts ? d : n_pts);
        }
        const int n_t = (n_eff + 31) >> 5, R = (n_t + DAL3_WG_WAVES - 1) / DAL3_WG_WAVES;
        float in[T][KS];
        load_points<KS, T>(x, b, R * wave * 32, n_eff, c_in, in, lane);  // (a point index beyond the item is clamped to its last point)
        for (int r = 0; r < R; ++r) {
            const int t = r + R * wave;
            const bool active = t < n_t;               // (wave-uniform; no early exit: every wave meets round 0's barrier)
            f32x16 x3[T][KT];
            if (active) {
                f32x16 x1[T][C1 / 32], x2[T][C2 / 32];
                first_layer<KS, C1 / 32, T>(w.w1, w.b1, in, x1, lane);
                mlp_layer_ring<C1 / 32, C2 / 32, T>(ring, w.b2, w.b3, bias, x1, x2, lane);
                mlp_layer_ring<C2 / 32, C3 / 32, T>(ring, w.b3, w.b2, bias, x2, x3, lane);   // leaves bias = conv2's tile 0
                load_points<KS, T>(x, b, (t + 1) * 32, n_eff, c_in, in, lane);               // the next round's points
                HSCR_COUNT(0, 1);
                HSTAMP(0);
                HSTAMP_ADD(8, 1u);
            }
            head_screen_tile<true>(w, w.stream + FRAGS23 * 64, r16, x3, t, n_eff, blob_dense, active, r == 0, r, L, wave, lane, st);
        }
        __syncthreads();                               // every wave's exact values are in the table
        i0 = threadIdx.x;
        asm volatile("" : "+v"(i0));
        for (int c = i0; c < 512; c += 64 * DAL3_WG_WAVES) gi[c] = L.tab[c];
        HSTAMP(6);
        // the next item. (A thread rewrites the table entries it has just flushed, no others; s_item is rewritten only
        // after the barrier above of the next item, which every thread reaches after reading it here.)
        if (threadIdx.x == 0) s_item = (int)(atomicAdd(cursor, 1u) + gridDim.x);
        __syncthreads();
        b = __builtin_amdgcn_readfirstlane(s_item);    // (uniform: the item's addresses and counts stay scalar)
        if (b >= B) break;
    }
#ifdef DAL3_STAMP
    if (lane == 0 && blockIdx.x * DAL3_WG_WAVES + wave < 1024) {
#pragma unroll
        for (int k = 0; k < 12; ++k) g_head_stamps[(blockIdx.x * DAL3_WG_WAVES + wave) * 16 + k] = st.acc[k];
    }
#endif
}

// cursor: one zeroable word of device scratch (the head's worklist, which this route does not build)
hipError_t launch_point_head_resident(int head_kind, const PointHeadW& w, BCN x, int c_in, int B, int M, float* feat,
                                      const int32_t* distinct, hipStream_t s, void* cursor, int cus) {
    if (!w.w4row || !w.w4h || !w.scr_pq || !w.scr_flag || !cursor || B < 1 || cus < 1) return hipErrorInvalidValue;
    const hipError_t e0 = hipMemsetAsync(cursor, 0, sizeof(uint32_t), s);
    if (e0 != hipSuccess) return e0;
    const dim3 grid((unsigned)(B < cus ? B : cus)), block(64 * DAL3_WG_WAVES);
    uint32_t* const cur = static_cast<uint32_t*>(cursor);
    switch (head_kind) {
        case 1:
            hipLaunchKernelGGL((point_head_resident_kernel<2, 128, 128, 256>), grid, block, 0, s, w, x, c_in, M, feat, distinct, B, cur);
            break;
        case 2:
            hipLaunchKernelGGL((point_head_resident_kernel<2, 64, 128, 256>), grid, block, 0, s, w, x, c_in, M, feat, distinct, B, cur);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_point_head_screen(int head_kind, const PointHeadW& w, BCN x, int c_in, float* feat, uint32_t* ctl,
                                    const u32x4* list, int64_t max_tiles, int64_t slots, hipStream_t s) {
    if (!w.w4row || !w.w4h || !w.scr_pq || !w.scr_flag) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(max_tiles < slots ? max_tiles : slots)), block(64);
    switch (head_kind) {
        case 1:
            hipLaunchKernelGGL((point_head_screen_kernel<2, 128, 128, 256>), grid, block, 0, s, w, x, c_in, feat, ctl, list);
            break;
        case 2:
            hipLaunchKernelGGL((point_head_screen_kernel<2, 64, 128, 256>), grid, block, 0, s, w, x, c_in, feat, ctl, list);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
