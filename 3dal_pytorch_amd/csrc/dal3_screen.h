// dal3_screen.h — the three primitives of a SCREENED max-pool (DESIGN.md "Screened conv5"): the compare of an fp16 score
// against its threshold, the candidate lists of a wave's tiles, and the exact fp32 recompute of one list.
//
// A wave sweeps NBLK blocks of 32 channels; lane l holds channel 32 mt + (l & 31) of block mt and, per tile j < T, the 16
// accumulator registers r (point tile_chan(r, l >> 5)). Per block the lane collects ONE hit word:
//   push number s = r * T + j (the order the slices visit the registers) ends at bit 16 T - 1 - s.
// The words are parked in LDS, [block][lane], and counted as they are made; the lists are built ONCE after the sweep:
// a wave prefix scan of the lanes' counts gives every lane the positions of its own entries. No ballot, no
// VALU -> scalar round trip and no branch rides in the sweep itself.
#pragma once
#include "dal3_device.h"


// Hit bit of one score: (hb << 1) | (acc > k). The sign of k - acc IS the comparison (no VCC, no select); it also lists
// acc = +0 against k = -0, a pair that is no candidate — harmless, its exact value goes to the same integer max. The set
// of listed pairs may grow and never shrinks: acc > k (both finite, |acc| <= 128 * 65504^2, |k| <= 3.0e38: no overflow
// to an infinity whose sign could lie) always gives a negative difference.
__device__ __forceinline__ uint32_t scr_push_hit(uint32_t hb, float acc, float k) {
    return __builtin_amdgcn_alignbit(hb, __float_as_uint(k - acc), 31);
}

// Order-preserving key of a SIGNED score for an unsigned atomic max (the maxima of dconv1a's fp16 scores, which the
// decoder's plan reads: DESIGN.md "Crop-dead channels of dconv1"): a < b as floats <=> key(a) < key(b), -0 below +0; 0 lies
// below the key of every finite value and of -Inf, so a zero-filled table is "nothing seen yet".
__host__ __device__ __forceinline__ uint32_t prune_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__host__ __device__ __forceinline__ uint32_t prune_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// bits of a hit word that belong to tile j: pushes s = j (mod T), bit 16 T - 1 - s
template <int T>
__host__ __device__ constexpr uint32_t scr_tile_mask(int j) {
    uint32_t m = 0;
    for (int s = j; s < 16 * T; s += T) m |= 1u << (16 * T - 1 - s);
    return m;
}

// A lane's running account of the sweep: its candidates per tile and which blocks hold any (block mt at bit
// NBLK - 1 - mt, shifted in like the hits).
template <int T>
struct ScreenHits {
    uint32_t n[T];
    uint32_t nz;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < T; ++j) n[j] = 0;
        nz = 0;
    }
    // hb: the block's hit word (bits from 16 T up are older pushes). park: the wave's NBLK * 64 words.
    __device__ __forceinline__ void park_block(uint32_t* park, int mt, uint32_t hb, int lane) {
        hb &= (uint32_t)((1ull << (16 * T)) - 1ull);
        park[mt * 64 + lane] = hb;
#pragma unroll
        for (int j = 0; j < T; ++j) n[j] += (uint32_t)__builtin_popcount(hb & scr_tile_mask<T>(j));
        nz = (nz << 1) | (hb < 1u ? hb : 1u);
    }
};

// The lists of the wave's T tiles from the parked words. cnt[j] (wave-uniform) is the tile's exact candidate count.
// Returns true, and writes NOTHING, if a tile has more than CAP candidates; otherwise list[j * CAP + 0 .. cnt[j]) holds
// every set bit of tile j once, as (channel << 8) | point, in no particular order.
template <int T, int NBLK, int CAP>
__device__ __forceinline__ bool scr_build_lists(const uint32_t* park, uint32_t* list, ScreenHits<T> hits, uint32_t (&cnt)[T], int lane) {
    static_assert(16 * T <= 32 && NBLK <= 32, "one hit word per block, one block bit per word");
    const int h = lane >> 5;
    uint32_t pos[T];
    bool overflow = false;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        uint32_t incl = hits.n[j];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            incl += lane >= d ? up : 0u;
        }
        pos[j] = incl - hits.n[j];
        cnt[j] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        overflow |= cnt[j] > (uint32_t)CAP;
    }
    if (overflow) return true;
    uint32_t nz = hits.nz, w = 0;
    int mt = 0;
    for (;;) {                                         // per lane: one entry per trip; a trip that starts a block reads its word
        if (w == 0) {
            if (nz == 0) break;
            mt = NBLK - 1 - __builtin_ctz(nz);
            nz &= nz - 1;
            w = park[mt * 64 + lane];
        }
        const int s = 16 * T - 1 - __builtin_ctz(w);
        w &= w - 1;
        const int j = s % T, r = s / T;
        const uint32_t e = ((uint32_t)(32 * mt + (lane & 31)) << 8) | (uint32_t)tile_chan(r, h);
        uint32_t at = 0;
#pragma unroll
        for (int jj = 0; jj < T; ++jj) {
            at = j == jj ? (uint32_t)(jj * CAP) + pos[jj] : at;
            pos[jj] += j == jj ? 1u : 0u;
        }
        list[at] = e;                                  // (at < j * CAP + cnt[j] <= (j + 1) * CAP: no tile overflows here)
    }
    return false;
}

// The exact recompute of one list over NS slices of SW input channels: one candidate per lane and round of 64, the
// dense kernel's chain — fmaf from a0 in the f32 MFMA's k order (channels 8i, 8i+4, 8i+1, 8i+5, ... of every group of 8),
// the operands x from the tile's point-major LDS copy (row stride xld floats) and w from wrow[channel * ldw ..].
// Only the DELIVERY of w differs from a per-lane row read: per slice, SW / 4 lanes fetch one candidate's SW floats (with
// SW = 32 a wave instruction touches 8 whole 128-byte lines, not 64 lines), the pieces go to a padded LDS row per
// candidate (SW + 4 words: rows 4 banks apart, the 64 ds_read_b128 of a row read conflict-free) and the lane reads its
// own row back. DEPTH slices are in flight at once (4 * SW / 4 * DEPTH registers), and a slice's registers are refilled
// as soon as they are staged, with the slice DEPTH further on — of the NEXT round at a round's end: in steady state no
// global round trip is exposed.
// EARLY reads the next round's list entries at the round's start (SW / 4 more registers) instead of where they are
// needed. a0(idx, live) gives the chain's start, fin(a, channel, idx, live) takes its end. cnt is wave-uniform; stage holds
// 64 * (SW + 4) words.
template <int SW, int NS, int DEPTH, bool EARLY, typename A0, typename Fin>
__device__ __forceinline__ void scr_recompute(const float* __restrict__ wrow, int ldw, const uint32_t* list, uint32_t cnt,
                                              const float* xw, int xld, uint32_t* stage, int lane, A0&& a0, Fin&& fin) {
    static_assert(SW == 16 || SW == 32, "a slice is 4 or 8 lanes of 16 bytes per candidate");
    static_assert(DEPTH >= 1 && NS % DEPTH == 0, "slices in flight: slice q lives in registers q % DEPTH, round after round");
    constexpr int LPC = SW / 4, LD = SW + 4;           // lanes per candidate = loads per slice; words per staged row
    const int sub = lane / LPC, piece = lane % LPC;
    u32x4 wq[DEPTH][LPC];
    uint32_t off[LPC], noff[EARLY ? LPC : 1];          // byte offsets from wrow (uniform base, 32-bit lane offset) of this lane's pieces: this round's, the next's
    auto served = [&](uint32_t base, uint32_t (&o)[LPC]) {
#pragma unroll
        for (int t = 0; t < LPC; ++t) {
            const uint32_t idx = base + (64 / LPC) * t + sub;
            o[t] = (list[idx < cnt ? idx : 0u] >> 8) * (uint32_t)(ldw * 4) + (uint32_t)(16 * piece);
        }
    };
    auto issue = [&](int q) {                          // slice q into the registers of slice q - DEPTH
#pragma unroll
        for (int t = 0; t < LPC; ++t) wq[q % DEPTH][t] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wrow) + (off[t] + (uint32_t)(4 * SW * q)));
    };
    if (cnt == 0) return;
    served(0, off);
#pragma unroll
    for (int q = 0; q < DEPTH; ++q) issue(q);
    for (uint32_t base = 0; base < cnt; base += 64) {
        const uint32_t idx = base + lane;
        const bool live = idx < cnt;
        const uint32_t e = list[live ? idx : 0u];
        const int c = (int)(e >> 8), p = (int)(e & 31u);
        const bool more = base + 64 < cnt;             // (uniform)
        if constexpr (EARLY) {                         // (read with the round's own entry: no wait of its own later)
            if (more) served(base + 64, noff);
        }
        const f32x4* xr = reinterpret_cast<const f32x4*>(xw + p * xld);
        float a = a0(idx, live);
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            __builtin_amdgcn_wave_barrier();           // (the previous slice's row reads are issued: LDS keeps a wave's order)
#pragma unroll
            for (int t = 0; t < LPC; ++t) *reinterpret_cast<u32x4*>(stage + ((64 / LPC) * t + sub) * LD + 4 * piece) = wq[q % DEPTH][t];
            __builtin_amdgcn_wave_barrier();
            if (q + DEPTH < NS) {
                issue(q + DEPTH);
            } else if (more) {
                if (q + DEPTH == NS) {                 // (this round's slices are all issued: the rows of the next)
                    if constexpr (EARLY) {
#pragma unroll
                        for (int t = 0; t < LPC; ++t) off[t] = noff[t];
                    } else {
                        served(base + 64, off);
                    }
                }
                issue(q + DEPTH - NS);
            }
            u32x4 wr[LPC];
#pragma unroll
            for (int i = 0; i < LPC; ++i) wr[i] = *reinterpret_cast<const u32x4*>(stage + lane * LD + 4 * i);
#pragma unroll
            for (int i = 0; i < LPC / 2; ++i) {
                const u32x4 w0 = wr[2 * i], w1 = wr[2 * i + 1];
                const f32x4 x0 = xr[LPC * q + 2 * i], x1 = xr[LPC * q + 2 * i + 1];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a = fmaf(x0[k], __uint_as_float(w0[k]), a);
                    a = fmaf(x1[k], __uint_as_float(w1[k]), a);
                }
            }
        }
        fin(a, c, idx, live);
    }
}
