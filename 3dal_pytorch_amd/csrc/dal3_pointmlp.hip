// dal3_pointmlp.hip — the per-point shared-MLP kernels (fp32 MFMA, activations in registers).
//
//   ins_seg_encode : conv1..conv5 + BN + ReLU, channel-wise max over N fused into conv5's epilogue
//                    (static_model.py:279-284) -> g (B,1024). The (B,1024,N) tensor never exists.
//   ins_seg_decode : recomputes conv1-2 from the points, then dconv1 (per-point 64->512 part; the
//                    global-feature part arrives as the per-crop vector gb) streamed in 32-channel
//                    chunks straight into dconv2's K loop, dconv3, dconv4, dconv5 + the '<' mask
//                    (static_model.py:286-295, :59) -> logits (B,N,2), mask (B,N).
//   point_head     : conv1..conv4 + max over M (static_model.py:330-334, dynamic_model.py:241-245,
//                    278-282) -> feat (B,512).
//
// One wave owns T tiles of 32 points; waves never talk to each other (no LDS, no barrier): the
// cross-wave max is an atomic on g / feat. Weights stream from L2 as 1-KiB coalesced dwordx4
// fragments shared by all waves of the chip. The one exception is ins_seg_decode_pair_kernel, the
// throughput decoder of large fp32 jobs: a pair of waves shares a tile, its row queue and barriers.
#include <stdlib.h>

#include <type_traits>

#include "dal3_device.h"
#include "dal3_kernels.h"

// Diagnostic build only (-DDAL3_STAMP): s_memtime stamps of the decode kernel's phases (0..4; the compacted body adds 5: dconv3's
// rows queued, 6: dconv3 done, 7: dconv4's rows queued; 8 + i / 11 + i: entry and exit of dconv2's group i < 3, 14: those groups'
// k-steps in bits 16 i ..), 16 words per wave, written to a buffer of their own (dal3_debug_set_stamps). No stamp executes in
// the shipped library.
#ifdef DAL3_STAMP
__device__ long long* g_stamps = nullptr;
extern "C" int dal3_debug_set_stamps(void* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &p, sizeof(p));
}
#define STAMP(k)                                                                                  \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        unsigned long long t_;                                                                    \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (lane == 0 && blockIdx.x < 2048) g_stamps[(blockIdx.x * DAL3_WG_WAVES + wave) * 16 + (k)] = t_; \
    } while (0)
#else
#define STAMP(k)
#endif

// ------------------------------------------------------------------------------------------------
// Every kernel reads its MFMA weights as ONE fragment stream in consumption order (see InsSegW /
// PointHeadW) through one prefetch ring that never restarts between layers.
#ifndef DAL3_ENC_LDS_MAX
#define DAL3_ENC_LDS_MAX 1              // 0: every wave's per-tile maxima straight to global memory (A/B builds)
#endif
template <int T>
__global__ __launch_bounds__(64 * DAL3_WG_WAVES) void ins_seg_encode_kernel(InsSegW w, BCN pts, int c_in, int n_pts,
                                                             int tiles_per_item, float* __restrict__ g) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = lane >> 5;
    const int64_t b = blockIdx.x / tiles_per_item;
    const int n0 = ((blockIdx.x % tiles_per_item) * DAL3_WG_WAVES + wave) * (32 * T);
    __shared__ float s_b5[1024];                       // conv5's folded bias, read by the max epilogue
    // The workgroup's maxima meet in LDS first (round 4): every wave used to send its 1024 per-channel maxima to the
    // crop's row of g with global atomics — 4 KiB of atomic traffic per 64 points, 268 MB per 4096 x 1024 launch for a
    // 16.8 MB result (16 x). The bit patterns are >= 0 after the ReLU, so the table starts at 0 and an
    // integer max is the float max; one global atomicMax per channel and WORKGROUP follows (none where the value is 0:
    // the caller zero-fills g).
    __shared__ int s_max[DAL3_ENC_LDS_MAX ? 1024 : 1];
    for (int i = threadIdx.x; i < 1024; i += 64 * DAL3_WG_WAVES) {
        s_b5[i] = w.b5[i];
        if (DAL3_ENC_LDS_MAX) s_max[i] = 0;
    }
    __syncthreads();
    if (n0 < n_pts) {                                  // (no early return: every wave meets the barrier below)
        WRing<DAL3_PF> ring;
        ring.init(w.enc_stream, lane);                 // conv2 | conv3 | conv4 | conv5
        f32x16 bias = tile_from_channels(w.b2, h);
        float in[T][2];
        load_points<2, T>(pts, b, n0, n_pts, c_in, in, lane);
        f32x16 x1[T][2], x2[T][2], x3[T][2], x4[T][4];
        first_layer<2, 2, T>(w.w1, w.b1, in, x1, lane);
        mlp_layer_ring<2, 2, T>(ring, w.b2, w.b3, bias, x1, x2, lane);
        mlp_layer_ring<2, 2, T>(ring, w.b3, w.b4, bias, x2, x3, lane);
        mlp_layer_ring<2, 4, T>(ring, w.b4, w.b4, bias, x3, x4, lane);
        conv_max_layer<4, T>(ring, s_b5, x4, DAL3_ENC_LDS_MAX ? reinterpret_cast<float*>(s_max) : g + b * 1024, 32, lane);
    }
    if (DAL3_ENC_LDS_MAX) {
        __syncthreads();
        int* gi = reinterpret_cast<int*>(g + b * 1024);
        for (int c = threadIdx.x; c < 1024; c += 64 * DAL3_WG_WAVES) {
            const int v = s_max[c];
            if (v > 0) atomicMax(gi + c, v);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Compacted dconv2 (DESIGN.md "Compacted dconv2"). dconv2's input is relu(dconv1), and on real crops almost half of a
// 32-channel chunk is +0 in all 32 points of a wave's tile (the per-crop term gb drives whole channels negative). A term
// fmaf(w, +0, acc) with finite w leaves acc as it is (up to the sign of a zero accumulator, which the ReLU after dconv2
// removes), so the dead channels are dropped from the k loop and every output keeps its chain of the live terms in the
// dense order — the same bits. dconv1 produces that input in chunks of 32 channels; the compact k-loop runs once per
// GROUP of DAL3_DEC_GROUP chunks (one start — list, first LDS and L2 round trips — per group instead of one per chunk).
// Per chunk, between the next chunk's dconv1 MFMAs: 16 wave ballots, collected in the lanes of one vector register and
// compared once (note_halves / live_word), give the live mask in chain order (bit 2r + h = accumulator register r, lane
// half h), kept as one scalar word, and the 16 registers go to rows 32 u + 2r + h
// of the wave's row queue in LDS (u: the chunk's place in its group; immediate offsets, no address arithmetic). Per
// group: the mask words become the LIST of live chain indices in chain order with v_mbcnt, 64 indices per pass; an entry
// is two words, the byte offset k * 1024 of the channel's weights and the float offset of its row. The leftover of the
// groups before, if any, is entry 0. Compact k-step s: half-wave h takes entry 2 s + h, reads that row as the B operand
// and 32 bytes per lane of the chain-ordered weight copy dw2c[k][row][out-tile] as the A operands of the step's eight
// MFMAs; a step's entry is read 2 DAL3_DEC_NB steps ahead, its row and weights DAL3_DEC_NB steps ahead (the two-stage
// loop of dec_queue_layer). An odd total leaves its last entry over: the row is copied to row DEC_G_PEND — the next
// groups overwrite the rows of this one, however many of them are entirely dead — and the entry goes first in the next
// list; the very last one is paired with the row of zeros. A fully live group is 16 DAL3_DEC_GROUP k-steps in the dense
// order; there is one route only.
// The weight ring of this body carries conv2 only: dconv1's A operands come from the chain-ordered copy dw1c, row by row
// of the crop's plan (see ins_seg_decode_tile), into the ring's eight slots.
// lanes whose post-ReLU bits are not +0: NaN and Inf are live. As asm: this file is built -fno-honor-nans, and hipcc turns
// the integer compare on the ReLU's result into v_cmp_lt_f32 0, v, which is false for a NaN.
__device__ __forceinline__ uint64_t live_ballot(float v) {
    uint64_t bal;
    asm("v_cmp_ne_u32_e64 %0, 0, %1" : "=s"(bal) : "v"(v));
    return bal;
}
// The live mask of 16 registers (32 rows: bit 2 r + h = register r, lane half h) from their ballots. A row is live if its
// half of the ballot is not 0. Taken on the scalar unit that is five instructions per register (two s_min_u32, a shift-add, a
// shift, an OR), and on this chip every instruction a wave issues between its fp32 MFMAs costs its issue time, scalar ones
// included (profiles/LEDGER_r15.md, section 2). Instead the two halves of ballot r go to lanes 2 r and 2 r + 1 of ONE vector
// register, two v_writelane_b32 with constant lane numbers, and one compare of that register at the end gives the word.
__device__ __forceinline__ void note_halves(uint32_t& halves, uint64_t bal, int r) {
    // (the scalar operand is the DATA: a vector compare's result needs wait states only in front of a lane SELECT)
    asm("v_writelane_b32 %0, %1, %3\n\tv_writelane_b32 %0, %2, %4"
        : "+v"(halves)
        : "s"((uint32_t)bal), "s"((uint32_t)(bal >> 32)), "n"(2 * r), "n"(2 * r + 1));
}
__device__ __forceinline__ uint32_t live_word(uint32_t halves) {   // (an integer compare: no NaN question; lanes 32 .. 63 hold 0)
    return (uint32_t)__builtin_amdgcn_ballot_w64(halves != 0u);
}
#ifndef DAL3_DEC_SPARSE
#define DAL3_DEC_SPARSE 1               // 0: every chunk on the dense path (A/B builds)
#endif
#ifndef DAL3_DEC_NB
#define DAL3_DEC_NB 3                   // compact k-steps whose operands are in flight (2 KiB of weights + one LDS row each)
#endif
#ifndef DAL3_DEC_GROUP
#define DAL3_DEC_GROUP 4                // dconv1 chunks per compact loop of dconv2: 2, 4 or 8
#endif
static_assert(DAL3_DEC_GROUP == 2 || DAL3_DEC_GROUP == 4 || DAL3_DEC_GROUP == 8,
              "a group's rows fit the queue's 256; the chunk loop goes in pairs, and the last group may be shorter");
static_assert(DAL3_PF == 8, "the compacted body's ring holds exactly one dconv1 chunk between two blocks");
// Diagnostic build only (-DDAL3_DEC_COUNT): [0] tiles, [1] dense chunks, [2] compacted chunks, [3] compact k-steps (the
// final zero-padded one included), [4] live channels, [5] tiles in the compacted body, [6] / [7] dconv3's compact k-steps and
// live rows, [8] / [9] dconv4's (compacted body only; `out` holds 12 words). No counter executes in the shipped library.
#ifdef DAL3_DEC_COUNT
__device__ unsigned long long g_dec_count[12];
extern "C" int dal3_debug_dec_counts(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dec_count), sizeof(g_dec_count));
    if (e == hipSuccess && reset) {
        unsigned long long z[12] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_dec_count), z, sizeof(z));
    }
    return (int)e;
}
#endif
struct DecStep {                        // operands of one compact k-step: weights of the 8 out-tiles, one activation
    f32x4 a0, a1;
    float b;
};

// Compacted dconv3 / dconv4 (DESIGN.md "Compacted dconv2 - dconv4"). The layer's whole input (KT accumulator tiles, post-ReLU)
// is complete when the layer starts, so it goes through ONE per-wave row queue in LDS and ONE compact k-loop with a single
// start. A row is one input channel's 32 points; row k of the queue is chain index k = 32 kt + 2 r + h (k-tile, accumulator
// register r, lane half h: the order of mlp_layer_ring's terms), so the 16 KT row writes need no address arithmetic. One
// wave ballot per register holds the two live bits as its halves; the halves of a k-tile's 16 ballots go to the lanes of one
// vector register and one compare of it gives the k-tile's mask word (note_halves / live_word: three vector instructions per
// register where the scalar unit took five and a wait), kept as a scalar (bit k of the layer's mask). The rows are written and
// the list is built BEFORE the loop starts: slicing the production by out-tile and running it between the k-steps of a loop
// that consumes the list as far as it is final was built and measured, and did not pay — a wave's instructions between its
// fp32 MFMAs cost their issue time there as they do here (profiles/LEDGER_r15.md, section 3).
// The mask then becomes the LIST of live chain indices in chain order, 64 indices per
// pass: lane L owns index 64 j + L, its place in the list is the number of live indices below it (v_mbcnt on the mask word
// plus the scalar count of the words before), and only live lanes write. Compact k-step s: half-wave h takes list entry
// 2 s + h, reads that row as its B operand and 16 bytes per lane of the chain-ordered weight copy [k][row 0..31][out-tile 0..3]
// as the A operands of the step's four MFMAs. An odd count ends on row 256, the row of zeros, whose weights lie past the
// copy's end and read as zeros. Every output keeps its chain of the live terms in the dense order.
// The loop runs two stages ahead of the MFMAs: a step's list entry is read 2 DAL3_DEC_QNB steps early, its row and weights
// DAL3_DEC_QNB steps early, so neither the LDS nor the L2 round trip is waited for. Entries past the list's end are the row
// of zeros (DEC_Q_OVER of them are written): every address stays inside the queue, and those operands are never multiplied.
#ifndef DAL3_DEC_QNB
#define DAL3_DEC_QNB 4                  // queue k-steps whose operands are in flight (1 KiB of weights + one LDS row each)
#endif
#define DEC_Q_ZERO 256                  // the row of zeros, behind the 256 rows of dconv3's input
#define DEC_Q_OVER 32                   // list entries past the end that the loop may read: 2 (2 DAL3_DEC_QNB) + 2 at the most
#define DEC_Q_LIST (256 + DEC_Q_OVER)
// dconv2's groups use rows 0 .. 32 DAL3_DEC_GROUP - 1 and the row of zeros, and behind dconv3's / dconv4's list a row and a
// list of their own: row DEC_G_PEND holds the leftover, the list has two words per entry (the leftover, a group's rows,
// DEC_Q_OVER entries behind the end)
#define DEC_G_PEND ((DEC_Q_ZERO + 1) + DEC_Q_LIST / 32)
#define DEC_G_LIST ((DEC_G_PEND + 1) * 32)                  // float offset of dconv2's list
#define DEC_Q_FLOATS (DEC_G_LIST + 2 * (1 + 256 + DEC_Q_OVER))   // rows | zeros | list | leftover row | dconv2's list
static_assert(DEC_Q_LIST % 32 == 0, "the leftover row starts where dconv3's list ends");
static_assert(4 * DAL3_DEC_QNB + 2 <= DEC_Q_OVER, "the loop reads list entries up to 2 (steps - 1 + 2 DAL3_DEC_QNB) + 1");
static_assert(4 * DAL3_DEC_NB + 2 <= DEC_Q_OVER, "dconv2's loop reads list entries up to 2 (steps - 1 + 2 DAL3_DEC_NB) + 1");
struct QStep {
    f32x4 a;
    float b;
};
template <int KT, int STAMP0>
__device__ __forceinline__ void dec_queue_layer(const f32x16 (&X)[KT], f32x16 (&Y)[4], const float* __restrict__ bvec,
                                                const float* __restrict__ wcopy, float* q, int lane, uint32_t& n_steps,
                                                uint32_t& n_live) {
    static_assert(KT % 2 == 0, "two k-tiles per 64-bit mask word");
    const uint32_t h = (uint32_t)lane >> 5, pt = (uint32_t)lane & 31u;
    uint32_t* kl = reinterpret_cast<uint32_t*>(q + (DEC_Q_ZERO + 1) * 32);
    const __amdgpu_buffer_rsrc_t wq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wcopy), 0, KT * 32 * 512, 0x00020000);
    f32x16 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = tile_from_channels(bvec + 32 * mt, (int)h);
    // (LDS operations of a wave execute in order: these rows never overtake the reads of whatever used the queue before)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint32_t m[KT];                                    // live mask, word kt: bit 2 r + h
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        uint32_t halves = 0;                           // lane 2 r + h: the ballot of register r in lane half h (see live_word)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = X[kt][r];
            q[(32 * kt + 2 * r) * 32 + lane] = v;      // rows 32 kt + 2 r (low half) and + 1 (high half)
            note_halves(halves, live_ballot(v), r);
        }
        m[kt] = live_word(halves);
    }
    q[DEC_Q_ZERO * 32 + pt] = 0.0f;
    uint32_t cnt = 0;                                  // live rows (wave-uniform)
#pragma unroll
    for (int j = 0; j < KT / 2; ++j) {
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(m[2 * j + 1], __builtin_amdgcn_mbcnt_lo(m[2 * j], 0u));
        const uint32_t word = h ? m[2 * j + 1] : m[2 * j];
        if ((word >> pt) & 1u) kl[cnt + below] = 64u * j + (uint32_t)lane;
        cnt += __builtin_popcount(m[2 * j]) + __builtin_popcount(m[2 * j + 1]);
    }
    if (lane < DEC_Q_OVER) kl[cnt + (uint32_t)lane] = DEC_Q_ZERO;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t steps = (cnt + 1u) >> 1;
    n_steps += steps, n_live += cnt;
#ifdef DAL3_STAMP
    const int wave = threadIdx.x >> 6;
    STAMP(STAMP0);
#endif
    auto mma = [&](const QStep& S) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = mfma32(S.a[mt], S.b, acc[mt]);
    };
    auto issue = [&](QStep& S, uint32_t k) {           // row k and its weights
        S.b = q[k * 32u + pt];
        S.a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wq, k * 512u + pt * 16u, 0, 0));
    };
    const uint32_t* kp = kl + h;                       // kp[2 t]: this half's chain index of step t
    QStep S[DAL3_DEC_QNB];
    uint32_t K[DAL3_DEC_QNB];
#pragma unroll
    for (int u = 0; u < DAL3_DEC_QNB; ++u) K[u] = kp[2 * u];
#pragma unroll
    for (int u = 0; u < DAL3_DEC_QNB; ++u) {
        issue(S[u], K[u]);
        K[u] = kp[2 * (DAL3_DEC_QNB + u)];
    }
    uint32_t s = 0;
    for (; s + DAL3_DEC_QNB <= steps; s += DAL3_DEC_QNB) {
        kp += 2 * DAL3_DEC_QNB;
#pragma unroll
        for (int u = 0; u < DAL3_DEC_QNB; ++u) {
            mma(S[u]);
            issue(S[u], K[u]);
            K[u] = kp[2 * (DAL3_DEC_QNB + u)];
            DAL3_SCHED_FENCE();
        }
    }
#pragma unroll
    for (int u = 0; u + 1 < DAL3_DEC_QNB; ++u) {
        if (s + u < steps) mma(S[u]);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) Y[mt] = relu16(acc[mt]);
}

// One wave's tile(s): SP = with the compacted dconv2 - dconv4 (slab: the wave's DEC_Q_FLOATS of LDS).
// SP runs dconv1 over the crop's PLAN (DESIGN.md "Crop-dead channels of dconv1"): pk[0 .. 32 nch) are the chain indices of the
// channels it computes, ascending and padded with the null channel, gbc their per-crop terms in row order, nch the chunk
// count (even). Row m = tile_chan(r, h) of chunk j is list entry 32 j + 2 r + h — the place the dense kernel gives that row —
// so registers, ballots, rows and list positions are those of a dense chunk and only the entry's dconv2 weight offset comes
// from the plan. A crop without a plan passes the identity (InsSegW::dec_ident, gb itself, 16 chunks). dconv1's A operands:
// a lane reads the 128 bytes of its row and k-half from the chain-ordered copy dw1c as eight 16-byte loads into the ring's
// slots, one chunk ahead; the row's chain index is read one chunk before that. The ring proper carries conv2 only.
template <int T, bool SP>
__device__ __forceinline__ void ins_seg_decode_tile(const InsSegW& w, const BCN& pts, int c_in, int n_pts, int64_t b, int n0,
                                                    const float* __restrict__ gb, float* __restrict__ logits,
                                                    uint8_t* __restrict__ mask, float* __restrict__ slab, int lane, int wave,
                                                    const uint32_t* __restrict__ pk = nullptr, const float* __restrict__ gbc = nullptr,
                                                    int nch = 16) {
    const int h = lane >> 5;
    STAMP(0);
    // stream: conv2 | dconv1a(0) | { dconv1a(c+1), dconv2(c) } c = 0..15 | dconv3 | dconv4
    WRing<DAL3_PF> ring;
    ring.init(w.dec_stream, lane);
    f32x16 bias = tile_from_channels(w.b2, h);
    // gb = W1g . g + b1' of this crop. A crop with a non-finite coordinate: its pooled feature, hence this term, is NaN
    // (dal3_device.h); as in the reference every logit of the crop is then NaN and its mask empty
    // (static_model.py:284-289, :59)
    const bool crop_bad = bits_nonfinite(gb[0]);

    const int pt = lane & 31;
    __amdgpu_buffer_rsrc_t wc = ring.rsrc;
    constexpr int G = DAL3_DEC_GROUP;
    constexpr int TRIP = SP ? G : 2;                   // chunks per trip of the chunk loop (the dense body's stays at two)
    uint32_t m[TRIP] = {};                             // SP: live mask of the trip's chunks, bit 2r + h
    uint32_t kq[TRIP / 2] = {};                        // SP: the plan's chain index of list position 64 j + lane of the trip
    uint32_t pend = 0;                                 // SP: an entry waits for a partner
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 pend_e = {0u, DEC_Q_ZERO * 32u};             // that entry: weight byte offset, float offset of row DEC_G_PEND
    u32x2* kl = reinterpret_cast<u32x2*>(slab + DEC_G_LIST);
    __amdgpu_buffer_rsrc_t wd1 = ring.rsrc;            // SP: dconv1a in chain order, 256 bytes per channel, the null channel last
    // SP: this lane's row of a chunk sits at list position 2 r + h, lane & 31 = tile_chan(r, h)
    const int row_pos = 2 * ((lane & 3) + 4 * ((lane & 31) >> 3)) + ((lane >> 2) & 1);
    uint32_t kf = 0, kn = 0;                           // SP: chain index of this lane's row in the chunk fetched next / after that
    if constexpr (SP) {
        wc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(w.dw2c), 0, 512 * 1024, 0x00020000);
        wd1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(w.dw1c), 0, (DEC_NULL_K + 1) * 256, 0x00020000);
        slab[DEC_Q_ZERO * 32 + pt] = 0.0f;
        kf = pk[row_pos];
        kn = pk[32 + row_pos];
    }
#ifdef DAL3_DEC_COUNT
    uint32_t n_dense = 0, n_comp = 0, n_steps = 0, n_live = 0;
#endif
#ifdef DAL3_STAMP
    unsigned long long stamp_steps = 0;
#endif

    f32x16 x2[T][2];
    {
        float in[T][2];
        load_points<2, T>(pts, b, n0, n_pts, c_in, in, lane);
        f32x16 x1[T][2];
        first_layer<2, 2, T>(w.w1, w.b1, in, x1, lane);
        if constexpr (SP) {
            // conv2 as mlp_layer_ring runs it, except that the second tile's block refills the slots with chunk 0 of dconv1
            f32x16 c2a[T], c2b[T];
            c2a[0] = bias;
            mma_block_ring<2, T>(ring, x1, c2a, [&](int i) {
                if (i == 0) bias = tile_from_channels(w.b2 + 32, h);
            });
            c2b[0] = bias;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 a = ring.slot[i];
                ring.slot[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wd1, kf * 256u + (uint32_t)h * 128u + 16u * i, 0, 0));
#pragma unroll
                for (int e = 0; e < 4; ++e) c2b[0] = mfma32(a[e], x1[0][i / 4][4 * (i % 4) + e], c2b[0]);
                DAL3_SCHED_FENCE();
                if (i == 0) bias = tile_from_channels(gbc, h);
                x2[0][0][2 * i] = relu1(c2a[0][2 * i]);
                x2[0][0][2 * i + 1] = relu1(c2a[0][2 * i + 1]);
                DAL3_SCHED_FENCE();
            }
            x2[0][1] = relu16(c2b[0]);
            kf = kn;
        } else {
            mlp_layer_ring<2, 2, T>(ring, w.b2, gb, bias, x1, x2, lane);   // leaves bias = gb chunk 0
        }
    }

    // dconv1 (512 outputs, 16 chunks of 32) streamed into dconv2 (256 outputs = 8 accumulator tiles).
    // dconv1 chunk c+1 is computed (into the other t buffer) BEFORE dconv2 consumes chunk c, and the
    // ReLU of chunk c rides under those MFMAs: no MFMA -> VALU -> MFMA bubble at the chunk seam.
    f32x16 a2[T][8];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        const f32x16 b2v = tile_from_channels(w.db2 + 32 * mt, h);
#pragma unroll
        for (int j = 0; j < T; ++j) a2[j][mt] = b2v;
    }
    STAMP(1);
    f32x16 tA[T], tB[T];
    auto dconv2_part = [&](const f32x16 (&t)[T]) {
#pragma unroll
        for (int i = 0; i < 32; ++i) {                 // fragment i of the chunk: out-tile i/4, q = i%4
            ring_batch_wait<DAL3_PF>(ring, i);
            const f32x4 a = ring.slot[i % DAL3_PF];
            ring.slot[i % DAL3_PF] = ring.fetch();
#ifdef DAL3_ABLATE_WINDOW
            ring.soff &= ~0x2000u;
#endif
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int j = 0; j < T; ++j) a2[j][i / 4] = mfma32(a[e], t[j][4 * (i % 4) + e], a2[j][i / 4]);
            }
            DAL3_SCHED_FENCE();
        }
    };
    auto compact_mma = [&](const DecStep& S) {
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) a2[0][mt] = mfma32(mt < 4 ? S.a0[mt & 3] : S.a1[mt & 3], S.b, a2[0][mt]);
    };
    // this lane's operands of list entry e: its row (B), 32 bytes of the channel's weights (A of the eight out-tiles)
    auto compact_issue = [&](DecStep& S, u32x2 e) {
        const uint32_t voff = e[0] + (uint32_t)pt * 32u;
        S.b = slab[e[1] + (uint32_t)pt];
        S.a0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wc, voff, 0, 0));
        S.a1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wc, voff + 16u, 0, 0));
    };
    // The group of chunks c0 .. c0 + NG - 1, whose rows are in the queue and whose masks are mg[0 .. NG - 1]
    auto dconv2_group = [&](auto ng, int c0, const uint32_t* mg) {
        constexpr int NG = decltype(ng)::value;        // G, or less for the crop's last group
#ifdef DAL3_STAMP
        if (c0 / G < 3) STAMP(8 + c0 / G);
#endif
        // (LDS operations of a wave execute in order: the next group's rows never overtake this group's reads)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        kl[0] = pend_e;                                // the leftover goes first (without one, entry 0 is written again below)
        uint32_t total = pend;
#pragma unroll
        for (int j = 0; j < (NG + 1) / 2; ++j) {       // 64 chain indices per pass: lane L owns 32 (c0 + 2j) + L
            const uint32_t w0 = mg[2 * j], w1 = 2 * j + 1 < NG ? mg[2 * j + 1] : 0u;
            const uint32_t below = __builtin_amdgcn_mbcnt_hi(w1, __builtin_amdgcn_mbcnt_lo(w0, 0u));
            const uint32_t word = h ? w1 : w0;
            if ((word >> pt) & 1u) {
                u32x2 e;
                e[0] = kq[j] * 1024u;                  // (without a plan: 32 (c0 + 2 j) + lane)
                e[1] = (64u * j + (uint32_t)lane) * 32u;
                kl[total + below] = e;
            }
            total += __builtin_popcount(w0) + __builtin_popcount(w1);
        }
        if (lane < DEC_Q_OVER) {                       // behind the end: the row of zeros (read ahead, never multiplied)
            u32x2 e;
            e[0] = 0u, e[1] = DEC_Q_ZERO * 32u;
            kl[total + (uint32_t)lane] = e;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t steps = total >> 1;
        const u32x2* kp = kl + h;                      // kp[2 t]: this half's entry of step t
        DecStep S[DAL3_DEC_NB];                        // operands in flight, rotating by name
        u32x2 K[DAL3_DEC_NB];
#pragma unroll
        for (int u = 0; u < DAL3_DEC_NB; ++u) K[u] = kp[2 * u];
#pragma unroll
        for (int u = 0; u < DAL3_DEC_NB; ++u) {
            compact_issue(S[u], K[u]);
            K[u] = kp[2 * (DAL3_DEC_NB + u)];
        }
        if (total & 1u) {
            // the last entry is left over: its row moves to row DEC_G_PEND behind the reads above (the only ones of that
            // row: a leftover is entry 0), before the next groups write over this group's rows
            pend_e = kl[total - 1u];
            const float v = slab[pend_e[1] + (uint32_t)pt];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            slab[DEC_G_PEND * 32 + pt] = v;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            pend_e[1] = DEC_G_PEND * 32u;
        }
        pend = total & 1u;
        uint32_t s = 0;
        for (; s + DAL3_DEC_NB <= steps; s += DAL3_DEC_NB) {
            kp += 2 * DAL3_DEC_NB;
#pragma unroll
            for (int u = 0; u < DAL3_DEC_NB; ++u) {
                compact_mma(S[u]);
                compact_issue(S[u], K[u]);
                K[u] = kp[2 * (DAL3_DEC_NB + u)];
                DAL3_SCHED_FENCE();
            }
        }
#pragma unroll
        for (int u = 0; u + 1 < DAL3_DEC_NB; ++u) {
            if (s + u < steps) compact_mma(S[u]);
        }
#ifdef DAL3_STAMP
        if (c0 / G < 3) {
            STAMP(11 + c0 / G);
            stamp_steps |= (unsigned long long)steps << (16 * (c0 / G));
        }
#endif
#ifdef DAL3_DEC_COUNT
        n_comp += NG, n_steps += steps;
#pragma unroll
        for (int j = 0; j < NG; ++j) n_live += __builtin_popcount(mg[j]);
#endif
    };
    // ONE route per body: the compacted body sends every chunk through the queue (a fully live group runs its k-steps in
    // the dense order), the dense body every chunk through the registers. A second route inside the compacted body made the
    // compiler move the dconv2 accumulators between two register sets at every chunk (profiles/LEDGER_r09.md).
    auto dconv2_chunk = [&](const f32x16 (&t)[T], int c, int u) {
#ifdef DAL3_DEC_COUNT
        ++n_dense, n_live += 32;
#endif
        dconv2_part(t);
    };
    // ReLU of two registers per fragment group; SP: their rows of the queue and their live bits (post-ReLU bits:
    // negatives and -0 are +0 already, NaN / Inf are live)
    uint32_t halves = 0;                               // SP: the ballots of the chunk whose ReLU is under way (see note_halves)
    auto relu_note = [&](f32x16& t, int i, int u) {
        t[2 * i] = relu1(t[2 * i]);
        t[2 * i + 1] = relu1(t[2 * i + 1]);
        if constexpr (SP) {
            if (i == 0) halves = 0;
#pragma unroll
            for (int r = 2 * i; r < 2 * i + 2; ++r) {
                const float v = t[r];
                slab[(32 * (u % G) + 2 * r) * 32 + lane] = v;          // rows 32 u + 2 r (low half) and + 1 (high half)
                note_halves(halves, live_ballot(v), r);                // bits 2 r and 2 r + 1 of the chunk's word
            }
            if (i == 7) m[u] = live_word(halves);
        }
    };
    // SP: one dconv1 block. The slots hold this chunk's rows; they are refilled with the next chunk's (this lane's row: chain
    // index kf), and the chain index of the row after that is asked for (chunk cn2 of the plan; the loop reads up to four
    // chunks past the crop's last one, which DEC_PLAN_LD holds: null channels, never used)
    auto dconv1_block = [&](f32x16& acc, int cn2, auto side) {
        const uint32_t voff = kf * 256u + (uint32_t)h * 128u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 a = ring.slot[i];
            ring.slot[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wd1, voff + 16u * i, 0, 0));
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma32(a[e], x2[0][i / 4][4 * (i % 4) + e], acc);
            DAL3_SCHED_FENCE();
            if (i == 0) kn = pk[32 * cn2 + row_pos];
            side(i);
            DAL3_SCHED_FENCE();
        }
        kf = kn;
    };
    if constexpr (SP) {
        tA[0] = bias;
        dconv1_block(tA[0], 2, [&](int i) {
            if (i == 0) bias = tile_from_channels(gbc + 32, h);
        });
        // chunks c, c + 1 of the crop's plan, at places u, u + 1 of their group
        auto pair = [&](int c, auto uc) {
            constexpr int u = decltype(uc)::value;
            tB[0] = bias;
            dconv1_block(tB[0], c + 3, [&](int i) {                     // chunk c+1; ReLU(chunk c) in its shadow
                if (i == 0) bias = tile_from_channels(gbc + 32 * (c + 2 < nch ? c + 2 : 0), h);
                if (i == 1) kq[(u / 2) % (TRIP / 2)] = pk[32 * c + lane];
                relu_note(tA[0], i, u);
            });
            tA[0] = bias;
            // chunk c+2 (behind the crop's last chunk: null channels or chunks the plan left out; the result is unused)
            dconv1_block(tA[0], c + 4, [&](int i) {
                if (i == 0) bias = c + 2 < nch ? tile_from_channels(gbc + 32 * (c + 3 < nch ? c + 3 : 0), h) : tile_from_channels(w.db3, h);
                relu_note(tB[0], i, u + 1);
            });
        };
        for (int c0 = 0; c0 < nch; c0 += G) {
            bool done = false;
#pragma unroll
            for (int u = 0; u < G; u += 2) {           // u: the pair's place in the group (a constant once unrolled)
                if (done) continue;
                if (u == 0) pair(c0, std::integral_constant<int, 0>());
                if (u == 2) pair(c0 + 2, std::integral_constant<int, 2>());
                if (u == 4) pair(c0 + 4, std::integral_constant<int, 4>());
                if (u == 6) pair(c0 + 6, std::integral_constant<int, 6>());
                if (u + 2 < G && c0 + u + 2 >= nch) {  // the crop's last group is shorter (wave-uniform)
                    if (u == 0) dconv2_group(std::integral_constant<int, 2>(), c0, m);
                    if (u == 2) dconv2_group(std::integral_constant<int, 4>(), c0, m);
                    if (u == 4) dconv2_group(std::integral_constant<int, 6>(), c0, m);
                    done = true;
                }
            }
            if (!done) dconv2_group(std::integral_constant<int, G>(), c0, m);
        }
    } else {
#pragma unroll
    for (int j = 0; j < T; ++j) tA[j] = bias;
    mma_block_ring<2, T>(ring, x2, tA, [&](int i) {
        if (i == 0) bias = tile_from_channels(gb + 32, h);
    });
    for (int c0 = 0; c0 < 16; c0 += TRIP) {
#pragma unroll
        for (int u = 0; u < TRIP; u += 2) {            // u: the chunk's place in the trip (a constant once unrolled)
            const int c = c0 + u;
#pragma unroll
            for (int j = 0; j < T; ++j) tB[j] = bias;
            mma_block_ring<2, T>(ring, x2, tB, [&](int i) {            // chunk c+1; ReLU(chunk c) in its shadow
                if (i == 0) bias = tile_from_channels(gb + 32 * ((c + 2) & 15), h);
#pragma unroll
                for (int j = 0; j < T; ++j) relu_note(tA[j], i, u);
            });
            dconv2_chunk(tA, c, u);
#pragma unroll
            for (int j = 0; j < T; ++j) tA[j] = bias;
            // chunk c+2 (on the last round its 8 fragments are the stream's zero filler; the result is unused)
            mma_block_ring<2, T>(ring, x2, tA, [&](int i) {
                if (i == 0)
                    bias = c + 2 < 16 ? tile_from_channels(gb + 32 * ((c + 3) & 15), h) : tile_from_channels(w.db3, h);
#pragma unroll
                for (int j = 0; j < T; ++j) relu_note(tB[j], i, u + 1);
            });
            dconv2_chunk(tB, c + 1, u + 1);
        }
    }
    }
    if constexpr (SP) {
        if (pend) {                                    // the very last live channel: its partner is the row of zeros
            DecStep S;
            u32x2 e = pend_e;
            if (h) e[1] = DEC_Q_ZERO * 32u;
            compact_issue(S, e);
            compact_mma(S);
#ifdef DAL3_DEC_COUNT
            ++n_steps;
#endif
        }
    }
#ifdef DAL3_DEC_COUNT
    if (lane == 0) {
        atomicAdd(&g_dec_count[0], 1ull);
        atomicAdd(&g_dec_count[5], SP ? 1ull : 0ull);
        atomicAdd(&g_dec_count[1], (unsigned long long)n_dense);
        atomicAdd(&g_dec_count[2], (unsigned long long)n_comp);
        atomicAdd(&g_dec_count[3], (unsigned long long)n_steps);
        atomicAdd(&g_dec_count[4], (unsigned long long)n_live);
    }
#endif
    STAMP(2);
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) a2[j][mt] = relu16(a2[j][mt]);
    }

    f32x16 y3[T][4], y4[T][4];
    if constexpr (SP) {                                // one route here too: both layers through the queue, even with nothing dead
        uint32_t q_steps3 = 0, q_live3 = 0, q_steps4 = 0, q_live4 = 0;
        dec_queue_layer<8, 5>(a2[0], y3[0], w.db3, w.dw3c, slab, lane, q_steps3, q_live3);
        STAMP(6);
        dec_queue_layer<4, 7>(y3[0], y4[0], w.db4, w.dw4c, slab, lane, q_steps4, q_live4);
#ifdef DAL3_DEC_COUNT
        if (lane == 0) {
            atomicAdd(&g_dec_count[6], (unsigned long long)q_steps3);
            atomicAdd(&g_dec_count[7], (unsigned long long)q_live3);
            atomicAdd(&g_dec_count[8], (unsigned long long)q_steps4);
            atomicAdd(&g_dec_count[9], (unsigned long long)q_live4);
        }
#endif
    } else {
        mlp_layer_ring<8, 4, T>(ring, w.db3, w.db4, bias, a2, y3, lane);
        mlp_layer_ring<4, 4, T>(ring, w.db4, w.db4, bias, y3, y4, lane);
    }

    STAMP(3);
    // dconv5 (128 -> 2, no BN/ReLU) on the VALU: each lane holds 64 of its point's 128 channels
    float l0[T], l1[T];
#pragma unroll
    for (int j = 0; j < T; ++j) l0[j] = l1[j] = 0.0f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 wa = *reinterpret_cast<const f32x4*>(w.dw5 + 32 * kt + 8 * q + 4 * h);
            const f32x4 wb = *reinterpret_cast<const f32x4*>(w.dw5 + 128 + 32 * kt + 8 * q + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    l0[j] = fmaf(wa[e], y4[j][kt][4 * q + e], l0[j]);
                    l1[j] = fmaf(wb[e], y4[j][kt][4 * q + e], l1[j]);
                }
            }
        }
    }
    const float bias0 = w.db5[0], bias1 = w.db5[1];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        float s0 = l0[j] + __shfl_xor(l0[j], 32) + bias0;
        float s1 = l1[j] + __shfl_xor(l1[j], 32) + bias1;
        if (crop_bad) s0 = s1 = __int_as_float(DAL3_QNAN_BITS);
        const int n = n0 + 32 * j + (lane & 31);
        if (h == 0 && n < n_pts) {
            f32x2 o;
            o[0] = s0;
            o[1] = s1;
            *reinterpret_cast<f32x2*>(logits + (b * n_pts + n) * 2) = o;
            mask[b * n_pts + n] = (!crop_bad && s0 < s1) ? 1 : 0;      // strict '<': ties are background
        }
    }
    STAMP(4);
#ifdef DAL3_STAMP
    if (lane == 0 && blockIdx.x < 2048) g_stamps[(blockIdx.x * DAL3_WG_WAVES + wave) * 16 + 14] = (long long)stamp_steps;
#endif
}

// The compacted body is taken by the tiles of a crop whose term gb is negative in at least DAL3_DEC_MIN_DEAD of the 512
// dconv1 channels — the channels that are dead for (nearly) every point of the crop — and never when the blob's guard
// flag is set. Every other tile runs the dense body, which is the kernel as it was: no ballot, no branch in its chunk
// loop. (The choice is about speed only: both bodies give the same bits. The compacted body sends every chunk, a fully
// live one included, through the queue: a crop with few dead channels would lose more to the ballots, the rows and the
// lists than compaction returns.)
// 64 = 0.125 of the channels is the smallest dead share with a measured gain: with exactly that share of dconv1 dead in every
// tile (the other channels live) the compacted body runs the 4096 x 1024 launch in 13.58 / 12.65 / 12.17 / 11.68 / 11.18 ms
// at 0 / 0.125 / 0.1875 / 0.25 / 0.3125 against 12.89 - 12.92 ms dense — break-even below 0.125; it was near 0.2 while dconv2's
// compact loop ran once per chunk (LEDGER_r12.md, section 3). With nothing dead it still loses 5 %: the dense body stays.
// A crop with a plan (DESIGN.md "Crop-dead channels of dconv1") is counted on the plan's flags, by dec_plan_kernel, against the
// same number: at exactly 64 flags the planned call is level with the unplanned one, at 128 it gains 0.35 ms (LEDGER_r14.md).
template <int T>
__global__ __launch_bounds__(64 * DAL3_WG_WAVES) void ins_seg_decode_kernel(InsSegW w, BCN pts, int c_in, int n_pts,
                                                             int tiles_per_item, const float* __restrict__ gbias,
                                                             float* __restrict__ logits, uint8_t* __restrict__ mask, DecPlan plan) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // Which (crop, tile) this workgroup takes. The hardware deals consecutive workgroup ids round-robin over the 8 XCDs,
    // each with an L2 of its own; with id -> (id / tiles_per_item, id % tiles_per_item) the 8 workgroups of a 1024-point
    // crop land on 8 different XCDs and each XCD's L2 fetches the crop's 2-KiB dconv1 term `gbias` from memory for itself:
    // 8 x 8.4 MB of the 130.7 MB this kernel read per 4096 x 1024 launch against 58.7 MB of points + terms (VERDICT r5 #6;
    // profiles/r06_pmc_decode_traffic.txt). Round 6: XCD x (ids = x mod 8) takes a CONTIGUOUS range of logical blocks, so a
    // crop's tiles share one L2. Pure index arithmetic; per-tile work is independent: bit-identical results.
#ifndef DAL3_DEC_XCD
#define DAL3_DEC_XCD 1
#endif
    unsigned blk = blockIdx.x;
    if (DAL3_DEC_XCD) {
        const unsigned per = gridDim.x >> 3, rem = gridDim.x & 7u, x = blockIdx.x & 7u;
        blk = x * per + (x < rem ? x : rem) + (blockIdx.x >> 3);
    }
    const int64_t b = blk / tiles_per_item;
    const int n0 = ((blk % tiles_per_item) * DAL3_WG_WAVES + wave) * (32 * T);
    if (n0 >= n_pts) return;
    const float* gb = gbias + b * 512;                 // W1g . g + b1' of this crop
    constexpr bool SP = DAL3_DEC_SPARSE != 0 && T == 1;    // one tile per wave only: the live mask is the tile's
    extern __shared__ __attribute__((aligned(16))) float s_slab[];   // SP: DAL3_WG_WAVES queues of DEC_Q_FLOATS (dynamic: above 64 KiB)
    if constexpr (SP) {
        // With a plan the dead channels are the plan's flags (dec_plan_kernel counts them: nch > 0 means at least
        // DAL3_DEC_MIN_DEAD and a clear guard flag); a crop without one is counted on gb and runs the identity plan.
        int nch = plan.nch ? plan.nch[b] : 0;
        const uint32_t* pk = plan.k + b * DEC_PLAN_LD;
        const float* gbc = plan.gbc + b * 512;
        bool sparse = nch > 0;
        if (!sparse) {
            const f32x4 g0 = reinterpret_cast<const f32x4*>(gb)[2 * lane], g1 = reinterpret_cast<const f32x4*>(gb)[2 * lane + 1];
            uint32_t neg = 0;                          // sign bits among the crop's 512 entries (a NaN term counts or not: dense either way is right)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                neg += __builtin_popcountll(__builtin_amdgcn_ballot_w64(__float_as_int(g0[e]) < 0)) +
                       __builtin_popcountll(__builtin_amdgcn_ballot_w64(__float_as_int(g1[e]) < 0));
            sparse = neg >= DAL3_DEC_MIN_DEAD && *w.dec_flag == 0;
            nch = 16, pk = w.dec_ident, gbc = gb;
        }
        if (sparse) {
            ins_seg_decode_tile<T, true>(w, pts, c_in, n_pts, b, n0, gb, logits, mask, s_slab + wave * DEC_Q_FLOATS, lane, wave, pk,
                                         gbc, nch);
            return;
        }
    }
    // The dense body starts on a 256-byte boundary of its own (the padding is s_nop, executed once per wave): its loops keep
    // their place relative to the instruction fetch windows whatever the length of the code in front of them. Without it
    // the same dense instructions ran 0.9 % slower once the prologue had become one scalar load shorter (LEDGER_r11.md, section 4).
    asm volatile(".p2align 8");
    ins_seg_decode_tile<T, false>(w, pts, c_in, n_pts, b, n0, gb, logits, mask, s_slab, lane, wave);
}

// ------------------------------------------------------------------------------------------------
// Two waves per tile (DESIGN.md "Two waves per tile"; tests/dec_pair_model.py is the schedule's CPU model). A workgroup is
// a PAIR of waves that owns one 32-point tile and runs the compacted body only; at 128 threads and at most 256 registers a
// CU holds four pairs, two waves on every SIMD, so the instructions one wave issues between its fp32 MFMAs lie beside the
// MFMAs of another. The two waves split every layer's OUTPUT tiles — dconv2's 4 w .. 4 w + 3 of eight, dconv3's and
// dconv4's 2 w, 2 w + 1 of four — and each runs the compact loop over the WHOLE list for its half: no output's chain is
// divided and every chain keeps the one-wave order, so the bits are ins_seg_decode_kernel's. What they share:
//   rows      dconv1's chunk j of the plan is computed by wave j mod 2 and written to rows 128 (g mod 2) + 32 u + 2 r + h
//             (group g = j / 4, place u = j mod 4): two buffers, rows 0 .. 127 and 128 .. 255. dconv3: wave w writes the
//             rows of its own four k-tiles (128 w ..), dconv4: of its own two (64 w ..). Wave 0 writes the row of zeros.
//   masks     a chunk's (k-tile's) producer leaves its mask word at a place of its own; dconv2's are double-buffered too.
//   barriers  one per group between its production and its consumption: produce(0) | B | consume(0) produce(1) | B | ... —
//             the producer of group g + 2 reaches buffer g mod 2 only after the barrier both waves pass once group g is
//             consumed. Then B | dconv3's rows | B | its loop | B | dconv4's rows | B | its loop, dconv5's first half | B |
//             dconv5's second half and the store. The pairs of a CU are separate workgroups and drift apart.
// Each wave has a list and a leftover row of ITS OWN (DEC_P_PRIV floats behind the shared rows): a shared leftover row
// would be overwritten by the faster wave's next odd group while the slower one still reads it as its list's entry 0.
// dconv5: one chain per logit and lane half in the one-wave order — wave 0 adds k-tiles 0, 1 from zero and hands the
// partial sums over in LDS, wave 1 CONTINUES them with k-tiles 2, 3, adds the lane halves and the bias, and stores.
// Each wave computes conv1 and conv2 for itself (68 of a tile's 1970 MFMAs twice). The ReLU, rows and ballots of a
// wave's second chunk of a group are not hidden under MFMAs of its own: the partner's are beside them.
// A blob whose guard flag is set is not for this kernel (every workgroup leaves at once): launch_ins_seg_decode puts
// ins_seg_decode_guarded_kernel behind it, which runs the dense body for such a blob and leaves at once for any other.
#define DEC_P_PRIV 612                                     // dconv2's list (dconv3's / dconv4's lie over it) | the leftover row
#define DEC_P_PEND_OFF (2 * (1 + 256 + DEC_Q_OVER))
#define DEC_P_LIST0 ((DEC_Q_ZERO + 1) * 32)
#define DEC_P_MASK (DEC_P_LIST0 + 2 * DEC_P_PRIV)          // 2 x 4 words of dconv2's groups, 8 of dconv3, 4 of dconv4
#define DEC_P_FLOATS (DEC_P_MASK + 32)
#define DEC_P_L5 (128 * 32)                                // dconv5's partial sums: rows that dconv4 does not use
static_assert(DEC_P_PEND_OFF + 32 <= DEC_P_PRIV && DEC_P_PRIV % 2 == 0 && DAL3_DEC_GROUP == 4, "the pair's LDS layout");
#ifdef DAL3_STAMP
// words per wave (blockIdx.x < 4096, wave 0 / 1): 0 start, 1 prologue done, 2 dconv2 done, 6 dconv3 done, 3 dconv4 done,
// 4 end; 8 ticks spent in barriers, 9 barriers, 10 k-steps of dconv2, 15 = 1 (tools/stamps.py --pair)
#define PSTAMP(k)                                                                                 \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        unsigned long long t_;                                                                    \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (lane == 0 && blockIdx.x < 4096) g_stamps[(blockIdx.x * 2 + wv) * 16 + (k)] = t_;      \
    } while (0)
#define PBARRIER()                                                                                \
    do {                                                                                          \
        unsigned long long t0_, t1_;                                                              \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0_)::"memory");              \
        __syncthreads();                                                                          \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1_)::"memory");              \
        bar_wait += t1_ - t0_, ++bar_n;                                                           \
    } while (0)
#else
#define PSTAMP(k)
#define PBARRIER() __syncthreads()
#endif
struct PStep {                          // operands of one compact k-step of dconv2 for four out-tiles
    f32x4 a;
    float b;
};
struct PQStep {                         // ... of dconv3 / dconv4 for two out-tiles
    f32x2 a;
    float b;
};
// dconv3 / dconv4 for wave wv of a pair: X its KT / 2 k-tiles of the input, Y its two out-tiles. kl: the wave's own list;
// mw: the layer's KT mask words. (dec_queue_layer with the rows and the out-tiles halved, and two barriers.)
template <int KT>
__device__ __forceinline__ void dec_pair_queue_layer(const f32x16 (&X)[KT / 2], f32x16 (&Y)[2], const float* __restrict__ bvec,
                                                     const float* __restrict__ wcopy, float* q, uint32_t* kl, uint32_t* mw, int lane,
                                                     uint32_t wv, uint32_t& n_steps, uint32_t& n_live, unsigned long long& bar_wait,
                                                     uint32_t& bar_n) {
    static_assert(KT % 4 == 0, "two k-tiles per 64-bit mask word, half of them per wave");
    const uint32_t h = (uint32_t)lane >> 5, pt = (uint32_t)lane & 31u;
    const __amdgpu_buffer_rsrc_t wq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wcopy), 0, KT * 32 * 512, 0x00020000);
    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[mt] = tile_from_channels(bvec + 32 * (2 * wv + mt), (int)h);
    PBARRIER();                                        // the partner has read what lay in these rows before
    float* qo = q + (KT / 2) * 1024 * wv + lane;       // the wave's own k-tiles: rows 32 (KT / 2 wv + i) + 2 r (+ 1: the high half)
#pragma unroll
    for (int i = 0; i < KT / 2; ++i) {
        uint32_t halves = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = X[i][r];
            qo[(32 * i + 2 * r) * 32] = v;
            note_halves(halves, live_ballot(v), r);
        }
        const uint32_t word = live_word(halves);
        if (lane == 0) mw[(KT / 2) * wv + i] = word;
    }
    PBARRIER();
    uint32_t m[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) m[kt] = __builtin_amdgcn_readfirstlane(mw[kt]);
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < KT / 2; ++j) {
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(m[2 * j + 1], __builtin_amdgcn_mbcnt_lo(m[2 * j], 0u));
        const uint32_t word = h ? m[2 * j + 1] : m[2 * j];
        if ((word >> pt) & 1u) kl[cnt + below] = 64u * j + (uint32_t)lane;
        cnt += __builtin_popcount(m[2 * j]) + __builtin_popcount(m[2 * j + 1]);
    }
    if (lane < DEC_Q_OVER) kl[cnt + (uint32_t)lane] = DEC_Q_ZERO;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t steps = (cnt + 1u) >> 1;
    n_steps += steps, n_live += cnt;
    auto mma = [&](const PQStep& S) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[mt] = mfma32(S.a[mt], S.b, acc[mt]);
    };
    auto issue = [&](PQStep& S, uint32_t k) {          // row k and its weights of the wave's two out-tiles
        S.b = q[k * 32u + pt];
        S.a = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(wq, k * 512u + pt * 16u + 8u * wv, 0, 0));
    };
    const uint32_t* kp = kl + h;
    PQStep S[DAL3_DEC_QNB];
    uint32_t K[DAL3_DEC_QNB];
#pragma unroll
    for (int u = 0; u < DAL3_DEC_QNB; ++u) K[u] = kp[2 * u];
#pragma unroll
    for (int u = 0; u < DAL3_DEC_QNB; ++u) {
        issue(S[u], K[u]);
        K[u] = kp[2 * (DAL3_DEC_QNB + u)];
    }
    uint32_t s = 0;
    for (; s + DAL3_DEC_QNB <= steps; s += DAL3_DEC_QNB) {
        kp += 2 * DAL3_DEC_QNB;
#pragma unroll
        for (int u = 0; u < DAL3_DEC_QNB; ++u) {
            mma(S[u]);
            issue(S[u], K[u]);
            K[u] = kp[2 * (DAL3_DEC_QNB + u)];
            DAL3_SCHED_FENCE();
        }
    }
#pragma unroll
    for (int u = 0; u + 1 < DAL3_DEC_QNB; ++u) {
        if (s + u < steps) mma(S[u]);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) Y[mt] = relu16(acc[mt]);
}

__global__ __launch_bounds__(128, 2) void ins_seg_decode_pair_kernel(InsSegW w, BCN pts, int c_in, int n_pts, int tiles_per_item,
                                                                     const float* __restrict__ gbias, float* __restrict__ logits,
                                                                     uint8_t* __restrict__ mask, DecPlan plan) {
    if (*w.dec_flag != 0) return;                      // (uniform: no wave of any workgroup reaches a barrier)
    const int lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, pt = lane & 31;
    unsigned blk = blockIdx.x;
    if (DAL3_DEC_XCD) {                                // a crop's workgroups share one XCD's L2 (see ins_seg_decode_kernel)
        const unsigned per = gridDim.x >> 3, rem = gridDim.x & 7u, x = blockIdx.x & 7u;
        blk = x * per + (x < rem ? x : rem) + (blockIdx.x >> 3);
    }
    const int64_t b = blk / tiles_per_item;
    const int n0 = (blk % tiles_per_item) * 32;
    const float* gb = gbias + b * 512;
    int nch = plan.nch ? plan.nch[b] : 0;
    const uint32_t* pk = plan.k + b * DEC_PLAN_LD;
    const float* gbc = plan.gbc + b * 512;
    if (nch <= 0) nch = 16, pk = w.dec_ident, gbc = gb;    // no plan: the identity, whatever the crop's dead share
    extern __shared__ __attribute__((aligned(16))) float s_slab[];
    float* slab = s_slab;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2* kl = reinterpret_cast<u32x2*>(slab + DEC_P_LIST0 + DEC_P_PRIV * wv);
    uint32_t* mw = reinterpret_cast<uint32_t*>(slab + DEC_P_MASK);
    const uint32_t pend_off = DEC_P_LIST0 + DEC_P_PRIV * wv + DEC_P_PEND_OFF;
    unsigned long long bar_wait = 0;
    uint32_t bar_n = 0;
    PSTAMP(0);

    WRing<DAL3_PF> ring;
    ring.init(w.dec_stream, lane);                     // conv2 only; dconv1's rows come from dw1c
    f32x16 bias = tile_from_channels(w.b2, h);
    const bool crop_bad = bits_nonfinite(gb[0]);
    const __amdgpu_buffer_rsrc_t wc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(w.dw2c), 0, 512 * 1024, 0x00020000);
    const __amdgpu_buffer_rsrc_t wd1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(w.dw1c), 0, (DEC_NULL_K + 1) * 256, 0x00020000);
    if (wv == 0) slab[DEC_Q_ZERO * 32 + pt] = 0.0f;
    const int row_pos = 2 * ((lane & 3) + 4 * ((lane & 31) >> 3)) + ((lane >> 2) & 1);
    // the wave's chunks are wv, wv + 2, ...: kf / kn the chain index of this lane's row in the chunk fetched next / after that
    uint32_t kf = pk[32 * wv + row_pos], kn = pk[32 * (wv + 2) + row_pos];
    f32x16 tA, tB;                                     // the wave's two chunks of a group; between groups: their terms gb
    f32x16 x2[1][2];
    {
        float in[1][2];
        load_points<2, 1>(pts, b, n0, n_pts, c_in, in, lane);
        f32x16 x1[1][2];
        first_layer<2, 2, 1>(w.w1, w.b1, in, x1, lane);
        f32x16 c2a[1], c2b[1];                         // conv2 as in ins_seg_decode_tile's compacted body
        c2a[0] = bias;
        mma_block_ring<2, 1>(ring, x1, c2a, [&](int i) {
            if (i == 0) bias = tile_from_channels(w.b2 + 32, h);
        });
        c2b[0] = bias;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 a = ring.slot[i];
            ring.slot[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wd1, kf * 256u + (uint32_t)h * 128u + 16u * i, 0, 0));
#pragma unroll
            for (int e = 0; e < 4; ++e) c2b[0] = mfma32(a[e], x1[0][i / 4][4 * (i % 4) + e], c2b[0]);
            DAL3_SCHED_FENCE();
            if (i == 0) tA = tile_from_channels(gbc + 32 * wv, h);
            if (i == 1) tB = tile_from_channels(gbc + 32 * (wv + 2 < (uint32_t)nch ? wv + 2 : 0), h);
            x2[0][0][2 * i] = relu1(c2a[0][2 * i]);
            x2[0][0][2 * i + 1] = relu1(c2a[0][2 * i + 1]);
            DAL3_SCHED_FENCE();
        }
        x2[0][1] = relu16(c2b[0]);
        kf = kn;
    }
    f32x16 a2[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) a2[mt] = tile_from_channels(w.db2 + 32 * (4 * wv + mt), h);
    PSTAMP(1);

    uint32_t halves = 0, kq0 = 0, kq1 = 0, pend = 0, n_steps = 0, n_live = 0;
    u32x2 pend_e = {0u, DEC_Q_ZERO * 32u};
    // ReLU of two registers, their rows (rows: the chunk's first row, this lane) and their live bits
    auto relu_note = [&](f32x16& t, int i, float* rows, uint32_t& word) {
        t[2 * i] = relu1(t[2 * i]);
        t[2 * i + 1] = relu1(t[2 * i + 1]);
        if (i == 0) halves = 0;
#pragma unroll
        for (int r = 2 * i; r < 2 * i + 2; ++r) {
            const float v = t[r];
            rows[2 * r * 32] = v;
            note_halves(halves, live_ballot(v), r);
        }
        if (i == 7) word = live_word(halves);
    };
    // one dconv1 chunk: the slots hold its rows and are refilled with the wave's next chunk's (chain index kf); jn: the chunk
    // after that, whose chain index is asked for (up to chunk 19 of the plan's 20: DEC_PLAN_LD)
    auto dconv1_block = [&](f32x16& acc, int jn, auto side) {
        const uint32_t voff = kf * 256u + (uint32_t)h * 128u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 a = ring.slot[i];
            ring.slot[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wd1, voff + 16u * i, 0, 0));
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma32(a[e], x2[0][i / 4][4 * (i % 4) + e], acc);
            DAL3_SCHED_FENCE();
            if (i == 0) kn = pk[32 * jn + row_pos];
            side(i);
            DAL3_SCHED_FENCE();
        }
        kf = kn;
    };
    // the group of chunks c0 .. c0 + 3 (c0 .. c0 + 1 for the plan's last two): this wave's are c0 + wv and c0 + 2 + wv
    auto produce = [&](int c0) {
        const uint32_t buf = ((uint32_t)c0 >> 2) & 1u;
        const bool two = c0 + 2 < nch;
        kq0 = pk[32 * c0 + lane];                      // the plan's chain index of list position 64 j + lane of the group
        kq1 = pk[32 * (c0 + 2) + lane];
        float* rows = slab + (128 * buf + 32 * wv) * 32 + lane;
        uint32_t mA = 0, mB = 0;
        dconv1_block(tA, c0 + (int)wv + 4, [](int) {});
        if (two) {
            dconv1_block(tB, c0 + (int)wv + 6, [&](int i) { relu_note(tA, i, rows, mA); });
#pragma unroll
            for (int i = 0; i < 8; ++i) relu_note(tB, i, rows + 64 * 32, mB);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) relu_note(tA, i, rows, mA);
        }
        if (lane == 0) {
            mw[4 * buf + wv] = mA;
            mw[4 * buf + 2 + wv] = mB;                 // (0 for a chunk behind the plan's last)
        }
        const int ja = c0 + 4 + (int)wv, jb = c0 + 6 + (int)wv;    // the next group's terms, into the registers just freed
        tA = tile_from_channels(gbc + 32 * (ja < nch ? ja : 0), h);
        tB = tile_from_channels(gbc + 32 * (jb < nch ? jb : 0), h);
    };
    auto compact_mma = [&](const PStep& S) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a2[mt] = mfma32(S.a[mt], S.b, a2[mt]);
    };
    auto compact_issue = [&](PStep& S, u32x2 e) {      // entry e: its row, and 16 bytes of the channel's weights (out-tiles 4 wv ..)
        S.b = slab[e[1] + (uint32_t)pt];
        S.a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wc, e[0] + (uint32_t)pt * 32u + 16u * wv, 0, 0));
    };
    auto consume = [&](int c0) {
        const uint32_t buf = ((uint32_t)c0 >> 2) & 1u;
        uint32_t mg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) mg[u] = __builtin_amdgcn_readfirstlane(mw[4 * buf + u]);
        kl[0] = pend_e;
        uint32_t total = pend;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t w0 = mg[2 * j], w1 = mg[2 * j + 1];
            const uint32_t below = __builtin_amdgcn_mbcnt_hi(w1, __builtin_amdgcn_mbcnt_lo(w0, 0u));
            const uint32_t word = h ? w1 : w0;
            if ((word >> pt) & 1u) {
                u32x2 e;
                e[0] = (j ? kq1 : kq0) * 1024u;
                e[1] = (128u * buf + 64u * j + (uint32_t)lane) * 32u;
                kl[total + below] = e;
            }
            total += __builtin_popcount(w0) + __builtin_popcount(w1);
        }
        if (lane < DEC_Q_OVER) {
            u32x2 e;
            e[0] = 0u, e[1] = DEC_Q_ZERO * 32u;
            kl[total + (uint32_t)lane] = e;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t steps = total >> 1;
        const u32x2* kp = kl + h;
        PStep S[DAL3_DEC_NB];
        u32x2 K[DAL3_DEC_NB];
#pragma unroll
        for (int u = 0; u < DAL3_DEC_NB; ++u) K[u] = kp[2 * u];
#pragma unroll
        for (int u = 0; u < DAL3_DEC_NB; ++u) {
            compact_issue(S[u], K[u]);
            K[u] = kp[2 * (DAL3_DEC_NB + u)];
        }
        if (total & 1u) {                              // the leftover moves to the wave's own row, behind the reads above
            pend_e = kl[total - 1u];
            const float v = slab[pend_e[1] + (uint32_t)pt];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            slab[pend_off + (uint32_t)pt] = v;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            pend_e[1] = pend_off;
        }
        pend = total & 1u;
        uint32_t s = 0;
        for (; s + DAL3_DEC_NB <= steps; s += DAL3_DEC_NB) {
            kp += 2 * DAL3_DEC_NB;
#pragma unroll
            for (int u = 0; u < DAL3_DEC_NB; ++u) {
                compact_mma(S[u]);
                compact_issue(S[u], K[u]);
                K[u] = kp[2 * (DAL3_DEC_NB + u)];
                DAL3_SCHED_FENCE();
            }
        }
#pragma unroll
        for (int u = 0; u + 1 < DAL3_DEC_NB; ++u) {
            if (s + u < steps) compact_mma(S[u]);
        }
        n_steps += steps;
#pragma unroll
        for (int u = 0; u < 4; ++u) n_live += __builtin_popcount(mg[u]);
    };
    produce(0);
    for (int c0 = 0; c0 < nch; c0 += 4) {
        PBARRIER();
        consume(c0);
        if (c0 + 4 < nch) produce(c0 + 4);
    }
    if (pend) {                                        // the very last live channel: its partner is the row of zeros
        PStep S;
        u32x2 e = pend_e;
        if (h) e[1] = DEC_Q_ZERO * 32u;
        compact_issue(S, e);
        compact_mma(S);
        ++n_steps;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) a2[mt] = relu16(a2[mt]);
    PSTAMP(2);
#ifdef DAL3_STAMP
    const unsigned long long stamp_steps2 = n_steps;
#endif

    f32x16 y3[2], y4[2];
    uint32_t q_steps3 = 0, q_live3 = 0, q_steps4 = 0, q_live4 = 0;
    uint32_t* ql = reinterpret_cast<uint32_t*>(kl);
    dec_pair_queue_layer<8>(a2, y3, w.db3, w.dw3c, slab, ql, mw + 8, lane, wv, q_steps3, q_live3, bar_wait, bar_n);
    PSTAMP(6);
    dec_pair_queue_layer<4>(y3, y4, w.db4, w.dw4c, slab, ql, mw + 16, lane, wv, q_steps4, q_live4, bar_wait, bar_n);
    PSTAMP(3);
#ifdef DAL3_DEC_COUNT
    if (lane == 0 && wv == 0) {
        atomicAdd(&g_dec_count[0], 1ull);
        atomicAdd(&g_dec_count[5], 1ull);
        atomicAdd(&g_dec_count[2], (unsigned long long)nch);
        atomicAdd(&g_dec_count[3], (unsigned long long)n_steps);
        atomicAdd(&g_dec_count[4], (unsigned long long)n_live);
        atomicAdd(&g_dec_count[6], (unsigned long long)q_steps3);
        atomicAdd(&g_dec_count[7], (unsigned long long)q_live3);
        atomicAdd(&g_dec_count[8], (unsigned long long)q_steps4);
        atomicAdd(&g_dec_count[9], (unsigned long long)q_live4);
    }
#endif

    // dconv5 on the VALU: the lane's chain runs over k-tiles 0 .. 3; wave 0 holds 0, 1 and starts it, wave 1 holds 2, 3
    float* l5 = slab + DEC_P_L5;
    float l0 = 0.0f, l1 = 0.0f;
    if (wv == 1) {
        PBARRIER();
        l0 = l5[lane], l1 = l5[64 + lane];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 wa = *reinterpret_cast<const f32x4*>(w.dw5 + 32 * (2 * wv + i) + 8 * q + 4 * h);
            const f32x4 wb = *reinterpret_cast<const f32x4*>(w.dw5 + 128 + 32 * (2 * wv + i) + 8 * q + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                l0 = fmaf(wa[e], y4[i][4 * q + e], l0);
                l1 = fmaf(wb[e], y4[i][4 * q + e], l1);
            }
        }
    }
    if (wv == 0) {
        l5[lane] = l0, l5[64 + lane] = l1;
        PBARRIER();
    } else {
        float s0 = l0 + __shfl_xor(l0, 32) + w.db5[0];
        float s1 = l1 + __shfl_xor(l1, 32) + w.db5[1];
        if (crop_bad) s0 = s1 = __int_as_float(DAL3_QNAN_BITS);
        const int n = n0 + pt;
        if (h == 0 && n < n_pts) {
            f32x2 o;
            o[0] = s0;
            o[1] = s1;
            *reinterpret_cast<f32x2*>(logits + (b * n_pts + n) * 2) = o;
            mask[b * n_pts + n] = (!crop_bad && s0 < s1) ? 1 : 0;      // strict '<': ties are background
        }
    }
    PSTAMP(4);
#ifdef DAL3_STAMP
    if (lane == 0 && blockIdx.x < 4096) {
        long long* st = g_stamps + (blockIdx.x * 2 + wv) * 16;
        st[8] = (long long)bar_wait, st[9] = bar_n, st[10] = (long long)stamp_steps2, st[15] = 1;
    }
#endif
}

// The dense body for a blob whose guard flag is set, behind ins_seg_decode_pair_kernel; any other blob: nothing to do.
__global__ __launch_bounds__(64 * DAL3_WG_WAVES) void ins_seg_decode_guarded_kernel(InsSegW w, BCN pts, int c_in, int n_pts,
                                                                                    int tiles_per_item, const float* __restrict__ gbias,
                                                                                    float* __restrict__ logits, uint8_t* __restrict__ mask) {
    if (*w.dec_flag == 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x / tiles_per_item;
    const int n0 = ((blockIdx.x % tiles_per_item) * DAL3_WG_WAVES + wave) * 32;
    if (n0 >= n_pts) return;
    ins_seg_decode_tile<1, false>(w, pts, c_in, n_pts, b, n0, gbias + b * 512, logits, mask, nullptr, lane, wave);
}

// ------------------------------------------------------------------------------------------------
template <int KS, int C1, int C2, int C3, int T>
__global__ __launch_bounds__(64 * DAL3_WG_WAVES) void point_head_kernel(PointHeadW w, BCN x, int c_in, int n_pts,
                                                         int tiles_per_item, float* __restrict__ feat,
                                                         const int32_t* __restrict__ distinct) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = lane >> 5;
    // item-minor block order: workgroups are dealt round-robin over the 8 XCDs, and with duplicate skipping only
    // an item's FIRST tiles carry work; (item, tile) = (id % B, id / B) spreads those over every XCD (with
    // item-major order and 4 tiles per item they all landed on 2 of the 8 XCDs: 4.6x slower)
    // ONE wave per workgroup: a wave that has nothing to do (below) exits at once, and inside a 4-wave workgroup its
    // SIMD would then idle until the slowest sibling is done (the workgroup keeps the CU: one wave per SIMD at this
    // register count) — 12 % of this kernel's time on the bench mix of crops.
    const int wg_waves = blockDim.x >> 6;
    const int n_items = gridDim.x / tiles_per_item;
    const int64_t b = blockIdx.x % n_items;
    const int n0 = ((blockIdx.x / n_items) * wg_waves + wave) * (32 * T);
    __shared__ float s_b4[512];                        // conv4's folded bias, read by the max epilogue
    for (int i = threadIdx.x; i < 512; i += blockDim.x) s_b4[i] = w.b4[i];
    __syncthreads();
    // distinct[b] (optional): only the first distinct[b] points of the item differ, the rest are duplicates of
    // them (gather: count < M tops up with copies; count == 0 is an all-zero row). The head is per-point work
    // followed by a max over points, so the duplicates cannot change the result and are not computed.
    if (distinct) {
        const int d = distinct[b];
        n_pts = d <= 0 ? 1 : (d < n_pts ? d : n_pts);
    }
    if (n0 >= n_pts) return;

    WRing<DAL3_PF> ring;
    ring.init(w.stream, lane);                         // conv2 | conv3 | conv4
    f32x16 bias = tile_from_channels(w.b2, h);
    f32x16 x3[T][C3 / 32];
    {
        float in[T][KS];
        load_points<KS, T>(x, b, n0, n_pts, c_in, in, lane);
        f32x16 x1[T][C1 / 32], x2[T][C2 / 32];
        first_layer<KS, C1 / 32, T>(w.w1, w.b1, in, x1, lane);
        mlp_layer_ring<C1 / 32, C2 / 32, T>(ring, w.b2, w.b3, bias, x1, x2, lane);
        mlp_layer_ring<C2 / 32, C3 / 32, T>(ring, w.b3, w.b3, bias, x2, x3, lane);
    }
    conv_max_layer<C3 / 32, T>(ring, s_b4, x3, feat + b * 512, 16, lane);
}

// ------------------------------------------------------------------------------------------------
// The point heads on a WORKLIST of live tiles (round 3). With the device sampler only the first min(count, M) object
// points of an item are distinct, so most items have tiles that hold nothing but copies; point_head_kernel above
// launches a one-wave workgroup for every (item, tile) and lets the dead ones exit — 26 % of the grid on the bench's mix
// of crops — and every live one pays its own launch, bias preload and cold weight ring for ONE 32-point tile (~90 us).
// Here the zero-fill of `feat` also turns `distinct` into the compacted list of (item, tile, points that count) entries, and
// persistent one-wave workgroups (as many as the chip holds at this register count) take entries from a device-side
// cursor: no dead workgroups, no relaunch, the weight ring runs on cyclically from tile to tile, and the next entry
// and its points are fetched while the current tile is computed. Per-point arithmetic and the atomicMax combine are
// those of point_head_kernel: bit-identical results (tests/test_gpu_parity.py). (The 16-bit heads were given the
// same list, in groups of 256 points, and timed both ways: 3.52 ms per C3 step either way — their kernel is persistent
// already and a group of copies is a uniform 1-us skip there — so they keep walking (item, group) pairs.)
//   ctl[0] = n_live, ctl[1] = cursor (zero), list[i] = {item, tile, n_eff, 0}: written by nonfinite_rows_kernel
//   (dal3_misc.hip), the launch that zero-fills `feat` in front of this kernel anyway
// Round 5: a wave takes RUNS of consecutive entries (the list is item-major, so a run is mostly one item's tiles) and
// keeps the item's 512 channel maxima in a private LDS row across the run; the global atomicMax is issued once per
// channel when the run leaves the item, not once per channel and TILE (rocprofv3 WRITE_SIZE: 108 MB per launch for an
// 8.4-MB result at 4096 x 512 object points, profiles/r04_pmc.json). Runs are HEAD_RUN entries long while plenty of
// work is left and shrink towards single entries at the end of the list (a run is the unit of the dynamic schedule:
// long runs at the end would leave waves idle for up to a run's time; guided self-scheduling: half of an even share of
// what is left). max is order-independent: bit-identical results.
#ifndef HEAD_RUN
#define HEAD_RUN 6
#endif
template <int KS, int C1, int C2, int C3>
__global__ __launch_bounds__(64) void point_head_pers_kernel(PointHeadW w, BCN x, int c_in, float* __restrict__ feat,
                                                             uint32_t* __restrict__ ctl, const u32x4* __restrict__ list) {
    constexpr int T = 1;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    __shared__ float s_b4[512];                        // conv4's folded bias, read by the max epilogue
    __shared__ int s_run[512];                         // the current item's channel maxima (bit patterns, >= 0)
    for (int i = threadIdx.x; i < 512; i += 64) {
        s_b4[i] = w.b4[i];
        s_run[i] = 0;
    }
    __syncthreads();
    const uint32_t n_live = ctl[0];
    // the schedule's cursor counts ENTRIES; the first gridDim.x * run0 entries are dealt out by block index. The first
    // run follows the same guided rule as every later one (round 6): half of an even share of the list, at most
    // HEAD_RUN, at least 1 — so a job of about one tile per wave (the reference's eval batch: 64 crops x 512 object
    // points = 1024 tiles) gives every wave ONE tile instead of six to a sixth of the chip (0.48 ms -> 0.1 ms there).
    uint32_t run0 = n_live / (2u * gridDim.x);
    run0 = run0 < 1u ? 1u : (run0 > HEAD_RUN ? HEAD_RUN : run0);
    const uint32_t first_free = gridDim.x * run0;
    uint32_t cur = blockIdx.x * run0, run_end = cur + run0;             // this wave's run: entries [cur, run_end)
    if (cur >= n_live) return;

    constexpr uint32_t STREAM_BYTES =
        ((C2 / 32) * (C1 / 32) + (C3 / 32) * (C2 / 32) + 16 * (C3 / 32)) * 4u * 1024u;   // conv2 | conv3 | conv4 fragments
    WRing<DAL3_PF, true> ring;
    ring.init(w.stream, lane, STREAM_BYTES);
    f32x16 bias = tile_from_channels(w.b2, h);
    u32x4 e = list[cur];
    float in[T][KS];
    load_points<KS, T>(x, (int64_t)e[0], (int)e[1] * 32, (int)e[2], c_in, in, lane);
    auto flush = [&](int64_t b) {                      // the finished item's maxima -> feat (nothing where the value is 0)
        int* gi = reinterpret_cast<int*>(feat + b * 512);
#pragma unroll
        for (int c = lane; c < 512; c += 64) {
            const int v = s_run[c];
            if (v > 0) atomicMax(gi + c, v);
            s_run[c] = 0;
        }
    };
    for (;;) {
        const int64_t b = (int64_t)e[0];
        // the run's last entry asks for the next run: one returning atomic, issued a whole layer before its result is
        // looked at (by then it is older than everything the ring has in flight, so the wait for it costs the ring
        // nothing). Its length: HEAD_RUN while more than 8 runs per wave are left behind the cursor, else 1.
        const bool last_of_run = cur + 1 >= run_end || cur + 1 >= n_live;
        uint32_t nxt = 0, take = 1;
        if (last_of_run) {
            const uint32_t left = n_live > run_end ? n_live - run_end : 0u;           // (behind this wave's own run: a proxy for the cursor)
            take = left / (2u * gridDim.x);                                           // guided: half of an even share of what is left
            take = take < 1u ? 1u : (take > HEAD_RUN ? HEAD_RUN : take);
            if (lane == 0) nxt = atomicAdd(&ctl[1], take);
        }
        f32x16 x3[T][C3 / 32];
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
            const uint32_t nclamp = ncur < n_live ? ncur : cur;        // (past the end: re-read this tile's entry, unused)
            e = list[nclamp];
            mlp_layer_ring<C2 / 32, C3 / 32, T>(ring, w.b3, w.b2, bias, x2, x3, lane);   // leaves bias = conv2's tile 0
            load_points<KS, T>(x, (int64_t)e[0], (int)e[1] * 32, (int)e[2], c_in, in_n, lane);
        }
        conv_max_layer<C3 / 32, T>(ring, s_b4, x3, reinterpret_cast<float*>(s_run), 16, lane);
        const bool more = ncur < n_live;
        if (!more || (int64_t)e[0] != b) flush(b);     // (the wave's own LDS operations are in order: no barrier)
        if (!more) break;
        cur = ncur;
        run_end = nend;
#pragma unroll
        for (int k = 0; k < KS; ++k) in[0][k] = in_n[0][k];
    }
}

// ------------------------------------------------------------------------------------------------
// One layer, any Cin = 32*KT (or a raw first layer when kt == 0 && ks > 0) -> y (B,N,Cout)
// point-major. Layer-wise test entry (dal3_shared_mlp_layer); not on the production path.
__global__ __launch_bounds__(256) void generic_layer_kernel(const f32x4* __restrict__ wf, const float* __restrict__ w1,
                                                            const float* __restrict__ bias, int kt_n, int ks_n, int mt_n,
                                                            int relu, BCN x, int c_in, int n_pts, int tiles_per_item,
                                                            float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = lane >> 5;
    const int64_t b = blockIdx.x / tiles_per_item;
    const int n0 = ((blockIdx.x % tiles_per_item) * 4 + wave) * 32;
    if (n0 >= n_pts) return;
    int n = n0 + (lane & 31);
    const bool valid = n < n_pts;
    n = valid ? n : n_pts - 1;
    const float* p = x.data + b * x.sb + (int64_t)n * x.sn;
    const int c_out = 32 * mt_n;
    for (int mt = 0; mt < mt_n; ++mt) {
        f32x16 acc = tile_from_channels(bias + 32 * mt, h);
        if (ks_n > 0) {
            for (int s = 0; s < ks_n; ++s) {
                const int c = 2 * s + h;
                const float bv = c < c_in ? p[c * x.sc] : 0.0f;
                acc = mfma32(w1[(mt * ks_n + s) * 64 + lane], bv, acc);
            }
        } else {
            for (int kt = 0; kt < kt_n; ++kt) {
                for (int q = 0; q < 4; ++q) {
                    const f32x4 a = wf[((mt * kt_n + kt) * 4 + q) * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = 32 * kt + 8 * q + 4 * h + e;
                        acc = mfma32(a[e], p[c * x.sc], acc);
                    }
                }
            }
        }
        if (relu) acc = relu16(acc);
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 o;
                o[0] = acc[4 * q + 0];
                o[1] = acc[4 * q + 1];
                o[2] = acc[4 * q + 2];
                o[3] = acc[4 * q + 3];
                *reinterpret_cast<f32x4*>(y + (b * n_pts + n) * c_out + 32 * mt + 8 * q + 4 * h) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
static inline int tiles_per_item(int n_pts, int T) {
    return (n_pts + 32 * DAL3_WG_WAVES * T - 1) / (32 * DAL3_WG_WAVES * T);
}

// Which family runs: the latency kernels (dal3_latency.hip: a 16-wave workgroup per tile, one per CU) while the job has
// at most DAL3_LAT_MAX_TILES tiles (512 = two rounds of workgroups on the 256 CUs), the throughput kernels above that.
// Both give the same bits. A pure function of the job and of the caller's flags (dal3.h: DAL3_BCN_NO_SMALL_JOB_KERNELS):
// no environment variable, no process-wide switch.
#ifndef DAL3_LAT_MAX_TILES
#define DAL3_LAT_MAX_TILES 512
#endif
#ifndef DAL3_LAT_MAX_TILES_ENC
#define DAL3_LAT_MAX_TILES_ENC DAL3_LAT_MAX_TILES
#endif
#ifndef DAL3_LAT_MAX_TILES_DEC
#define DAL3_LAT_MAX_TILES_DEC DAL3_LAT_MAX_TILES
#endif
#ifndef DAL3_LAT_MAX_TILES_HEAD
#define DAL3_LAT_MAX_TILES_HEAD DAL3_LAT_MAX_TILES
#endif
bool lat_use(int64_t tiles, int flags, int64_t max_tiles) { return !(flags & DAL3_BCN_NO_SMALL_JOB_KERNELS) && tiles <= max_tiles; }

// Do the screened encoder and the throughput decoder's compacted body both run for this job? Then the encoder leaves the
// bound of dconv1's crop-dead channels and the decoder takes a plan (dal3_api.hip: ins_seg_run). DAL3_BCN_NO_DEC_PLAN: never.
bool dec_plan_route(int flags, int B, int N) {
    const int64_t tiles = (int64_t)B * ((N + 31) / 32);
    if (flags & DAL3_BCN_NO_DEC_PLAN) return false;
    if (!DAL3_ENC_SCREEN || !DAL3_DEC_SPARSE || DAL3_DEC_T != 1) return false;
    if (lat_use(tiles, flags, DAL3_LAT_MAX_TILES_ENC) || lat_use(tiles, flags, DAL3_LAT_MAX_TILES_DEC)) return false;
    return !(DAL3_ENC_T > 1 && (int64_t)B * N <= 1024 * 64);
}

// The screened encoder as one crop-resident launch (dal3_enc_screen.hip): when the job has at least
// DAL3_ENC_RES_MIN_PER_CU whole-crop workgroups per CU; below that the two launches, whose workgroups are a quarter of a
// short crop. A pure function of B, the CU count and the caller's flags (dal3.h: DAL3_BCN_NO_ENC_RESIDENT selects the two
// launches for any job). Both give the same bits.
// Measured (profiles/LEDGER_r16.md, 256 CUs, encoder ms resident / two launches): a round of 256 whole-crop workgroups
// costs 0.76 of the two launches' time for 256 crops, so a batch a little above a whole number of rounds pays a nearly
// empty extra round: 300 x 1024 0.388 / 0.345 and 513 x 5120 2.320 / 2.110 lose (the edge at 1 and at 2 per CU); from 3 per
// CU nothing measured loses — 769 x 5120 3.180 / 3.168 is level within its spread of 0.044, 769 x 1024 0.757 / 0.816,
// 1025 x 5120 3.896 / 4.173, 4096 x 1024 3.149 / 4.035.
#ifndef DAL3_ENC_RES_MIN_PER_CU
#define DAL3_ENC_RES_MIN_PER_CU 3
#endif
static int enc_cu_count() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        n = v;
    }
    return n;
}
bool enc_resident_route(int flags, int B, int N) {
    (void)N;
    return !(flags & DAL3_BCN_NO_ENC_RESIDENT) && (int64_t)B >= (int64_t)DAL3_ENC_RES_MIN_PER_CU * enc_cu_count();
}
// Which fp32 encoder launch_ins_seg_encode takes (dal3.h: dal3_ins_seg_encoder_route), in the order it decides.
int enc_route(int flags, int B, int N) {
    if (lat_use((int64_t)B * ((N + 31) / 32), flags, DAL3_LAT_MAX_TILES_ENC)) return DAL3_ENC_ROUTE_LATENCY;
    if (DAL3_ENC_T > 1 && (int64_t)B * N <= 1024 * 64) return DAL3_ENC_ROUTE_DENSE;
    if (!DAL3_ENC_SCREEN) return DAL3_ENC_ROUTE_DENSE;
    return enc_resident_route(flags, B, N) ? DAL3_ENC_ROUTE_RESIDENT : DAL3_ENC_ROUTE_TWO_LAUNCH;
}

hipError_t launch_ins_seg_encode(const InsSegW& w, BCN pts, int c_in, int B, int N, float* g, hipStream_t s, uint32_t* prune) {
    if (lat_use((int64_t)B * ((N + 31) / 32), pts.flags, DAL3_LAT_MAX_TILES_ENC)) return launch_ins_seg_encode_lat(w, pts, c_in, B, N, g, s);
    constexpr int T = DAL3_ENC_T;
    // A wave runs its T tiles through the whole encoder one after the other (~150 us per tile at 2.4 GHz). When the
    // job cannot fill the chip's 1024 SIMDs anyway (small eval batches), one tile per wave halves that serial
    // chain; per-point arithmetic and the atomicMax combine are the same, so the result is bit-identical.
    if (T > 1 && (int64_t)B * N <= 1024 * 64) {
        const int tpi1 = tiles_per_item(N, 1);
        hipLaunchKernelGGL(ins_seg_encode_kernel<1>, dim3((unsigned)((int64_t)B * tpi1)), dim3(64 * DAL3_WG_WAVES), 0, s, w, pts, c_in, N, tpi1, g);
        return hipGetLastError();
    }
    // large jobs: conv5 screened in fp16, candidates recomputed exactly (dal3_enc_screen.hip); the same bits
    if (DAL3_ENC_SCREEN) return launch_ins_seg_encode_screen(w, pts, c_in, B, N, g, s, prune);
    const int tpi = tiles_per_item(N, T);
    hipLaunchKernelGGL(ins_seg_encode_kernel<T>, dim3((unsigned)((int64_t)B * tpi)), dim3(64 * DAL3_WG_WAVES), 0, s, w, pts, c_in, N, tpi, g);
    return hipGetLastError();
}

// The throughput decoder as pairs of waves (ins_seg_decode_pair_kernel): every job of the throughput family, unless the
// caller's flags say otherwise (dal3.h: DAL3_BCN_NO_DEC_PAIR selects ins_seg_decode_kernel for any job). A pure function of
// the job and the flags; both give the same bits. The blob's guard flag lives in device memory, so the decision about it is
// taken on the device: see ins_seg_decode_guarded_kernel. DAL3_DEC_PAIR_MIN_TILES: the smallest job that takes the pairs
// (profiles/LEDGER_r19.md).
#ifndef DAL3_DEC_PAIR
#define DAL3_DEC_PAIR 1                 // 0: never (A/B builds)
#endif
#ifndef DAL3_DEC_PAIR_MIN_TILES
#define DAL3_DEC_PAIR_MIN_TILES 0
#endif
bool dec_pair_route(int flags, int B, int N) {
    const int64_t tiles = (int64_t)B * ((N + 31) / 32);
    if (!DAL3_DEC_PAIR || (flags & DAL3_BCN_NO_DEC_PAIR)) return false;
    if (!DAL3_DEC_SPARSE || DAL3_DEC_T != 1) return false;
    if (lat_use(tiles, flags, DAL3_LAT_MAX_TILES_DEC)) return false;
    return tiles >= DAL3_DEC_PAIR_MIN_TILES;
}
// Which fp32 decoder launch_ins_seg_decode takes (dal3.h: dal3_ins_seg_decode_route); guarded: the blob's guard flag is set.
int dec_route(int flags, int B, int N, bool guarded) {
    if (lat_use((int64_t)B * ((N + 31) / 32), flags, DAL3_LAT_MAX_TILES_DEC)) return DAL3_DEC_ROUTE_LATENCY;
    return dec_pair_route(flags, B, N) && !guarded ? DAL3_DEC_ROUTE_PAIR : DAL3_DEC_ROUTE_ONE_WAVE;
}

hipError_t launch_ins_seg_decode(const InsSegW& w, BCN pts, int c_in, int B, int N, const float* gbias,
                                 float* logits, uint8_t* mask, hipStream_t s, DecPlan plan) {
    if (lat_use((int64_t)B * ((N + 31) / 32), pts.flags, DAL3_LAT_MAX_TILES_DEC)) return launch_ins_seg_decode_lat(w, pts, c_in, B, N, gbias, logits, mask, s);
    constexpr int T = DAL3_DEC_T;
    const int tpi = tiles_per_item(N, T);
    if (dec_pair_route(pts.flags, B, N)) {
        constexpr size_t lds_pair = (size_t)DEC_P_FLOATS * sizeof(float);
        const int tpi1 = (N + 31) / 32;
        hipLaunchKernelGGL(ins_seg_decode_pair_kernel, dim3((unsigned)((int64_t)B * tpi1)), dim3(128), lds_pair, s, w, pts, c_in, N, tpi1,
                           gbias, logits, mask, plan);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ins_seg_decode_guarded_kernel, dim3((unsigned)((int64_t)B * tpi)), dim3(64 * DAL3_WG_WAVES), 0, s, w, pts, c_in,
                           N, tpi, gbias, logits, mask);
        return hipGetLastError();
    }
    // the compacted body's row queues: one per wave, above the 64 KiB a kernel may take without asking
    constexpr size_t lds = DAL3_DEC_SPARSE != 0 && T == 1 ? (size_t)DAL3_WG_WAVES * DEC_Q_FLOATS * sizeof(float) : 0;
    if (lds) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ins_seg_decode_kernel<T>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ins_seg_decode_kernel<T>, dim3((unsigned)((int64_t)B * tpi)), dim3(64 * DAL3_WG_WAVES), lds, s, w, pts, c_in, N, tpi,
                       gbias, logits, mask, plan);
    return hipGetLastError();
}

// bytes of the worklist a launch_point_head of (B items, M points) may need: ctl (2 words, padded) + one entry per tile
size_t point_head_worklist_bytes(int B, int M) { return 256 + (size_t)B * ((M + 31) / 32) * sizeof(u32x4); }

// persistent one-wave workgroups the CURRENT device holds at this kernel's register count (one wave per SIMD): 4 per
// CU. Asked per call: hipGetDevice + hipDeviceGetAttribute are host-side table lookups (~0.1 us), and a process that
// drives several devices gets each one's own count.
static int head_slots() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
        v = 256;
    return 4 * v;
}

// The screened conv4 as one item-resident launch (dal3_head_screen.hip, point_head_resident_kernel): the heads with conv4
// 256 -> 512, items of more than one tile, when the job has at least DAL3_HEAD_RES_MIN_PER_CU items per CU of the current
// device; below that the two launches and their DAL3_HEAD_SCR_MIN_TILES, as before. A pure function of the job, the CU
// count and the caller's flags (dal3.h: DAL3_BCN_NO_HEAD_RESIDENT selects the two launches for any job). Both give the
// same bits. The constants are MEASURED (profiles/LEDGER_r18.md, "route constant"; 256 CUs, ms resident / two launches,
// bench mix of distinct points). box_est at B x 512: a CU takes whole items one after the other, so a batch a little above
// a whole number of items per CU pays for one more — with one workgroup per item 257 0.346 / 0.277 and 513 0.518 / 0.439
// lose (256 0.198 / 0.273 and 512 0.387 / 0.436 win); from 3 per CU, with the cursor grid, nothing measured loses: 768
// 0.553 / 0.608, 769 0.555 / 0.610, 1023 0.695 / 0.784, 1025 0.696 / 0.791, 4096 2.434 / 2.758. point_emb at B x 2560 (80
// tiles an item, one workgroup per item): 768 1.876 / 1.794 and 769 2.135 / 1.813 lose, 1024 2.468 / 2.489 is level within
// its spread of 0.024: from 4 per CU.
#ifndef DAL3_HEAD_RES_MIN_PER_CU
#define DAL3_HEAD_RES_MIN_PER_CU 3
#endif
#ifndef DAL3_HEAD_RES_MIN_PER_CU_EMB
#define DAL3_HEAD_RES_MIN_PER_CU_EMB 4
#endif
bool head_resident_route(int flags, int head_kind, int B, int M) {
    if (!DAL3_HEAD_SCREEN || DAL3_HEAD_T != 1 || (flags & (DAL3_BCN_NO_HEAD_RESIDENT | DAL3_BCN_NO_WORKLIST))) return false;
    if ((head_kind != 1 && head_kind != 2) || (M + 31) / 32 <= 1) return false;
    if (lat_use((int64_t)B * ((M + 31) / 32), flags, DAL3_LAT_MAX_TILES_HEAD)) return false;
    return (int64_t)B >= (int64_t)(head_kind == 1 ? DAL3_HEAD_RES_MIN_PER_CU : DAL3_HEAD_RES_MIN_PER_CU_EMB) * (head_slots() / 4);
}
// Which kernels launch_point_head takes when it is given a worklist (dal3.h: dal3_point_head_route), in the order it decides.
int head_route(int flags, int head_kind, int B, int M) {
    const int64_t tiles = (int64_t)B * ((M + 31) / 32);
    if (lat_use(tiles, flags, DAL3_LAT_MAX_TILES_HEAD)) return DAL3_HEAD_ROUTE_LATENCY;
    if ((flags & DAL3_BCN_NO_WORKLIST) || DAL3_HEAD_T != 1) return DAL3_HEAD_ROUTE_PER_TILE;
    if (head_resident_route(flags, head_kind, B, M)) return DAL3_HEAD_ROUTE_RESIDENT;
    if (DAL3_HEAD_SCREEN && (head_kind == 1 || head_kind == 2) && tiles >= DAL3_HEAD_SCR_MIN_TILES && (M + 31) / 32 > 1)
        return DAL3_HEAD_ROUTE_TWO_LAUNCH;
    return DAL3_HEAD_ROUTE_PERSISTENT;
}

hipError_t launch_point_head(int head_kind, const PointHeadW& w, BCN x, int c_in, int B, int M, float* feat,
                             const int32_t* distinct, hipStream_t s, void* worklist, size_t worklist_bytes) {
    constexpr int T = DAL3_HEAD_T;
    const int tpi = (M + 32 * T - 1) / (32 * T);       // one-wave workgroups
    const bool lat = lat_use((int64_t)B * ((M + 31) / 32), x.flags, DAL3_LAT_MAX_TILES_HEAD);
    const bool pers = !lat && worklist && worklist_bytes >= point_head_worklist_bytes(B, M) && !(x.flags & DAL3_BCN_NO_WORKLIST) && T == 1;
    // conv4 screened (dal3_head_screen.hip): whole items per workgroup where the job fills the chip with them (they read
    // `distinct` themselves: no worklist is built, its first word is the item cursor) ...
    const bool resident = pers && w.w4row && head_resident_route(x.flags, head_kind, B, M);
    // ... else the persistent route of a head with conv4 256 -> 512 from DAL3_HEAD_SCR_MIN_TILES tiles upward, and items
    // of more than one seed's worth of tiles
    const bool screen = DAL3_HEAD_SCREEN && pers && !resident && (head_kind == 1 || head_kind == 2) && w.w4row &&
                        (int64_t)B * tpi >= DAL3_HEAD_SCR_MIN_TILES && tpi > 1;
    // feat = 0 (NaN rows for items with a non-finite input, dal3.h) and, for the persistent kernel, the worklist
    hipError_t e0 = launch_nonfinite_rows(x, B, M, c_in, feat, 512, s, distinct, pers && !resident ? worklist : nullptr,
                                          screen ? DAL3_HEAD_SCR_STRIDE : 0);
    if (e0 != hipSuccess) return e0;
    if (resident) return launch_point_head_resident(head_kind, w, x, c_in, B, M, feat, distinct, s, worklist, head_slots() / 4);
    if (lat) return launch_point_head_lat(head_kind, w, x, c_in, B, M, feat, distinct, s);
    if (pers) {
        uint32_t* ctl = static_cast<uint32_t*>(worklist);
        u32x4* list = reinterpret_cast<u32x4*>(static_cast<char*>(worklist) + 256);
        const int64_t slots = head_slots();
        // (tile counts are upper bounds: the lists hold the live tiles only; a wave beyond its list exits)
        const int64_t seed_tpi = (tpi + DAL3_HEAD_SCR_STRIDE - 1) / DAL3_HEAD_SCR_STRIDE;
        const int64_t tiles = screen ? (int64_t)B * seed_tpi : (int64_t)B * tpi;
        const dim3 grid((unsigned)(tiles < slots ? tiles : slots)), block(64);
        switch (head_kind) {
            case 1:
                hipLaunchKernelGGL((point_head_pers_kernel<2, 128, 128, 256>), grid, block, 0, s, w, x, c_in, feat, ctl, list);
                break;
            case 2:
                hipLaunchKernelGGL((point_head_pers_kernel<2, 64, 128, 256>), grid, block, 0, s, w, x, c_in, feat, ctl, list);
                break;
            case 3:
                hipLaunchKernelGGL((point_head_pers_kernel<4, 64, 64, 128>), grid, block, 0, s, w, x, c_in, feat, ctl, list);
                break;
            default:
                return hipErrorInvalidValue;
        }
        hipError_t e1 = hipGetLastError();
        if (e1 != hipSuccess || !screen) return e1;
        // the seed launch above has left exact maxima in feat (same stream): the other live tiles, screened against them
        return launch_point_head_screen(head_kind, w, x, c_in, feat, ctl + 2, list + (size_t)B * seed_tpi,
                                        (int64_t)B * (tpi - seed_tpi), slots, s);
    }
    const dim3 grid((unsigned)((int64_t)B * tpi)), block(64);
    switch (head_kind) {
        case 1:  // static box_est 3 -> 128 -> 128 -> 256 -> 512
            hipLaunchKernelGGL((point_head_kernel<2, 128, 128, 256, T>), grid, block, 0, s, w, x, c_in, M, tpi, feat, distinct);
            break;
        case 2:  // point_emb 4 -> 64 -> 128 -> 256 -> 512
            hipLaunchKernelGGL((point_head_kernel<2, 64, 128, 256, T>), grid, block, 0, s, w, x, c_in, M, tpi, feat, distinct);
            break;
        case 3:  // box_emb 8 -> 64 -> 64 -> 128 -> 512
            hipLaunchKernelGGL((point_head_kernel<4, 64, 64, 128, T>), grid, block, 0, s, w, x, c_in, M, tpi, feat, distinct);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_generic_layer(const f32x4* wf, const float* w1, const float* bias, int kt_n, int ks_n, int mt_n,
                                int relu, BCN x, int c_in, int B, int N, float* y, hipStream_t s) {
    const int tpi = (N + 127) / 128;
    hipLaunchKernelGGL(generic_layer_kernel, dim3((unsigned)((int64_t)B * tpi)), dim3(256), 0, s, wf, w1, bias, kt_n,
                       ks_n, mt_n, relu, x, c_in, N, tpi, y);
    return hipGetLastError();
}
