// dal3_block.h — what the run kernels (dal3_motion.hip, dal3_track.hip, dal3_nms.hip, dal3_pillars.hip) share: the
// workspace carver, the grid clamp, the integer workgroup primitives of their ordered compactions, radix sorts and
// scans, the float64 fixed-tree workgroup sum of the loss and training kernels, the two binary searches, and the chunked radix sort of (key, position) pairs that the grouping run and the
// voxeliser both stand on. Everything here is used at two or more call sites; a building block with one user stays in
// its file. A run kernel's workspace size is its carve on a null base (Carver::off), never a formula of its own.
//
// The block primitives take their LDS arrays from the caller, must be called by every thread of the workgroup
// (they hold barriers) and index by threadIdx.x; waves are 64 lanes.
//
// dal3_nms.hip's sort is deliberately not the chunked sort: it is one workgroup per segment with the histogram in LDS,
// a different shape. It shares radix_tile_step and nothing above it.
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

// The grid of a launch that wants `want` workgroups: at least one, at most the site's `ceiling`, and at most
// max_workgroups when that is positive (the run kernels' argument; 0 leaves the grid to the site).
constexpr int64_t GRID_MAX = 0x7fffffff;        // the ceiling of a site that has none of its own: the launch limit
inline unsigned grid_clamp(int64_t want, int64_t ceiling, int64_t max_workgroups) {
    int64_t g = want < ceiling ? want : ceiling;
    if (g < 1) g = 1;
    if (max_workgroups > 0 && g > max_workgroups) g = max_workgroups;
    return (unsigned)g;
}

// The first index in [lo, hi) with v[i] >= x, and the first with v[i] > x; hi when there is none. v ascends.
template <typename T, typename X>
__device__ __forceinline__ int64_t lower_bound(const T* v, int64_t lo, int64_t hi, X x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename T, typename X>
__device__ __forceinline__ int64_t upper_bound(const T* v, int64_t lo, int64_t hi, X x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

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

// The float64 sum of one value per thread of a workgroup of `width` threads (a power of two) in a fixed tree: halves
// from width / 2 down to 1, so the bits depend on nothing but the values. Every thread gets the sum; s[width] is free
// again on return. `width` is a constant at most call sites and folds.
__device__ __forceinline__ double block_sum_f64(double v, double* s, int width) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = width >> 1; off > 0; off >>= 1) {
        if (t < off) s[t] += s[t + off];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
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

// ---------------------------------------------------------------------------------- chunked radix sort
// A stable least-significant-digit radix sort of n (key, position) pairs by their non-negative 32-bit keys, 8 bits a
// pass, over many workgroups. The input is cut into chunks of RADIX_CHUNK consecutive entries, whatever the grid; per pass
//   hist     each chunk's digit counts (LDS integer adds), stored digit-major (256, chunks);
//   scan     one exclusive scan over that table: where each (digit, chunk) run starts in the output;
//   scatter  each chunk again, tile by tile of RADIX_BLOCK consecutive entries on radix_tile_step: equal digits keep
//            their input order, so the pass is stable and the passes together sort by key with the positions ascending
//            inside a key.
// Every count is an integer and every output slot is a function of the input alone: no result depends on the grid,
// on which workgroup ran which chunk, or on the order atomics arrive in.
//
// The kernels are templates (on the key type; the scan on its block) in an unnamed namespace: a translation unit that
// sorts instantiates its own device copy, one that does not has none, and the objects link without relocatable device
// code.
namespace {

constexpr int RADIX_BLOCK = 256;
constexpr int RADIX_WAVES = RADIX_BLOCK / 64;
constexpr int RADIX_TILES = 16;
constexpr int64_t RADIX_CHUNK = (int64_t)RADIX_BLOCK * RADIX_TILES;     // 4096 entries
constexpr int RADIX_SCAN_BLOCK = 1024;

__host__ __device__ inline int64_t radix_chunks(int64_t n) { return (n + RADIX_CHUNK - 1) / RADIX_CHUNK; }

inline int radix_passes(int64_t max_key) {      // keys lie in [0, max_key]
    int bits = 1;
    while (bits < 32 && (max_key >> bits) != 0) ++bits;
    return (bits + 7) / 8;
}

template <typename K>
struct RadixBufs {
    K* key[2];                                  // (n) each: the pairs' keys, ping-pong; the input is key[0]
    int32_t* pos[2];                            // (n) each: the pairs' positions, ping-pong
    int32_t* hist;                              // (256, chunks)
};

// key[0], key[1], the first n_pos position buffers, hist, in this order. The position buffers it does not take
// (null here) are the caller's to set.
template <typename K>
inline RadixBufs<K> carve_radix(Carver& c, int64_t n, int n_pos) {
    RadixBufs<K> b = {};
    for (int i = 0; i < 2; ++i) b.key[i] = c.take<K>((size_t)n);
    for (int i = 0; i < n_pos; ++i) b.pos[i] = c.take<int32_t>((size_t)n);
    b.hist = c.take<int32_t>((size_t)256 * (size_t)radix_chunks(n));
    return b;
}

template <typename K>
__global__ __launch_bounds__(RADIX_BLOCK) void radix_hist_kernel(const K* key, int64_t E, int shift, int32_t* hist) {
    __shared__ int32_t s_hist[256];
    const int64_t chunks = radix_chunks(E);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        s_hist[threadIdx.x] = 0;
        __syncthreads();
        const int64_t e0 = c * RADIX_CHUNK;
        for (int r = 0; r < RADIX_TILES; ++r) {
            const int64_t i = e0 + (int64_t)r * RADIX_BLOCK + threadIdx.x;
            if (i < E) atomicAdd(&s_hist[(key[i] >> shift) & 255], 1);   // an integer count: the order does not matter
        }
        __syncthreads();
        hist[(int64_t)threadIdx.x * chunks + c] = s_hist[threadIdx.x];
        __syncthreads();
    }
}

// in-place exclusive scan of n int32 by ONE workgroup; total (optional) gets the sum
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void scan_kernel(int32_t* data, int64_t n, int64_t* total) {
    __shared__ int64_t s_part[BLOCK];
    const int64_t sum = block_scan_spans<BLOCK>(data, n, s_part);
    if (total && threadIdx.x == BLOCK - 1) *total = sum;
}

// pos_in == nullptr: the first pass, the position is the index itself
template <typename K>
__global__ __launch_bounds__(RADIX_BLOCK) void radix_scatter_kernel(const K* key_in, const int32_t* pos_in, int64_t E, int shift,
                                                                    const int32_t* hist, K* key_out, int32_t* pos_out) {
    __shared__ int32_t s_base[256];             // where the chunk's next entry of each digit goes
    __shared__ int32_t s_wave[RADIX_WAVES][256];    // the tile's count of each digit, per wave
    const int t = threadIdx.x;
    const int64_t chunks = radix_chunks(E);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        s_base[t] = hist[(int64_t)t * chunks + c];
        const int64_t e0 = c * RADIX_CHUNK;
        for (int r = 0; r < RADIX_TILES; ++r) {
            const int64_t i = e0 + (int64_t)r * RADIX_BLOCK + t;
            const bool live = i < E;
            const K k = live ? key_in[i] : 0;
            const int64_t o = radix_tile_step<RADIX_WAVES>(live, (k >> shift) & 255, s_base, s_wave);
            if (o >= 0 && o < E) {              // live; the bound always holds for a table hist/scan made from these keys
                key_out[o] = k;
                pos_out[o] = pos_in ? pos_in[i] : (int32_t)i;
            }
            __syncthreads();
        }
    }
}

// Sorts the n > 0 keys in b.key[0], each paired with its index, in `passes` passes on `grid` workgroups. The sorted
// pairs end in key[passes & 1] / pos[passes & 1]: pass p reads buffer p & 1 and writes the other one. The first pass
// takes the index itself as the position, so pos[0] is never read before it is written.
template <typename K>
inline hipError_t radix_sort_pairs(const RadixBufs<K>& b, int64_t n, int passes, unsigned grid, hipStream_t s) {
    const int64_t chunks = radix_chunks(n);
    for (int p = 0; p < passes; ++p) {
        const int in = p & 1, out = in ^ 1;
        hipLaunchKernelGGL(radix_hist_kernel<K>, dim3(grid), dim3(RADIX_BLOCK), 0, s, b.key[in], n, 8 * p, b.hist);
        hipLaunchKernelGGL(scan_kernel<RADIX_SCAN_BLOCK>, dim3(1), dim3(RADIX_SCAN_BLOCK), 0, s, b.hist, 256 * chunks, (int64_t*)nullptr);
        hipLaunchKernelGGL(radix_scatter_kernel<K>, dim3(grid), dim3(RADIX_BLOCK), 0, s, b.key[in],
                           p ? b.pos[in] : (const int32_t*)nullptr, n, 8 * p, b.hist, b.key[out], b.pos[out]);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace
