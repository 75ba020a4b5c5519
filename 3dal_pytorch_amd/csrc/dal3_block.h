// dal3_block.h — what the run kernels (dal3_motion.hip, dal3_track.hip, dal3_nms.hip) share: the workspace carver
// and the integer workgroup primitives of their ordered compactions, radix sorts and scans. Everything here is used
// at two or more call sites; a building block with one user stays in its file. A run kernel's workspace size is
// its carve on a null base (Carver::off), never a formula of its own.
//
// The block primitives take their LDS arrays from the caller, must be called by every thread of the workgroup
// (they hold barriers) and index by threadIdx.x; waves are 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

__host__ __device__ inline size_t ws_align(size_t b) { return (b + 255) & ~(size_t)255; }

// Hands out consecutive 256-byte-padded arrays of a workspace. A null base gives null pointers and only counts:
// `off` is then the size the workspace needs. `ok` turns false when the arrays do not fit into `size` bytes.
struct Carver {
    char* base;
    size_t size, off;
    bool ok;
    __host__ __device__ Carver(void* p, size_t n) : base(static_cast<char*>(p)), size(n), off(0), ok(true) {}
    template <typename T>
    __host__ __device__ T* take(size_t count) {
        const size_t bytes = ws_align(count * sizeof(T));
        char* p = base ? base + off : nullptr;
        off += bytes;
        if (base && off > size) ok = false;
        return reinterpret_cast<T*>(p);
    }
};

// Ordered compaction: the exclusive rank of `flag` among the workgroup's WAVES * 64 threads, in thread order, and
// the workgroup's count. s_cnt[WAVES] is free again on return.
template <int WAVES>
__device__ __forceinline__ int32_t block_rank(bool flag, int32_t* s_cnt, int32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int32_t in_wave = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        before += w < wave ? s_cnt[w] : 0;
        total += s_cnt[w];
    }
    __syncthreads();
    return before + in_wave;
}

// One tile of a stable radix scatter pass: thread t holds entry t of a tile of WAVES * 64 consecutive entries
// (`live`: it is one) with the 8-bit digit d. s_base[256] is where the next entry of each digit goes. An entry's rank
// among the tile's equal digits comes from wave ballots and the waves' counts in wave order, so equal digits keep
// their input order. Returns the entry's destination (-1 when not live) and advances s_base past the tile; the
// caller needs a barrier before anything but the next tile's call touches s_base.
template <int WAVES>
__device__ __forceinline__ int64_t radix_tile_step(bool live, int d, int32_t* s_base, int32_t (*s_wave)[256]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s_wave[w][t] = 0;
    __syncthreads();                            // s_base / the zeroes are in place
    // the lanes of this wave that hold the same digit
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    const int32_t before = __popcll(peers & ((1ull << lane) - 1ull));
    if (live && before == 0) s_wave[wave][d] = __popcll(peers);
    __syncthreads();
    int64_t o = -1;
    if (live) {
        int32_t off = before;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) off += w < wave ? s_wave[w][d] : 0;
        o = (int64_t)s_base[d] + off;
    }
    __syncthreads();                            // every read of s_base is done
    int32_t add = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) add += s_wave[w][t];
    s_base[t] += add;
    return o;
}

// In-place inclusive Hillis-Steele scan of s[BLOCK], thread t = element t. The caller's barrier after writing s
// comes first; s is complete for every thread on return.
template <int BLOCK, typename T>
__device__ __forceinline__ void block_scan_inclusive(T* s) {
    const int t = threadIdx.x;
    for (int off = 1; off < BLOCK; off <<= 1) {
        const T add = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
}

// In-place exclusive scan of n int32 by ONE workgroup of BLOCK threads: thread t owns the contiguous span
// [t * per, (t + 1) * per). Returns the total (to every thread); s_part[BLOCK] is read until then, so a caller that
// loops puts a barrier before the next call.
template <int BLOCK>
__device__ __forceinline__ int64_t block_scan_spans(int32_t* data, int64_t n, int64_t* s_part) {
    const int t = threadIdx.x;
    const int64_t per = (n + BLOCK - 1) / BLOCK;
    const int64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += data[i];
    s_part[t] = sum;
    __syncthreads();
    block_scan_inclusive<BLOCK>(s_part);        // of the spans' sums
    int64_t run = s_part[t] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t v = data[i];
        data[i] = (int32_t)run;
        run += v;
    }
    return s_part[BLOCK - 1];
}
