// dal3_nms.hip — the detector's post-processing (dal3_nms / dal3_center_decode / dal3_center_decode_flip4 /
// dal3_flip4_points, include/dal3.h): the non-maximum
// suppression of det3d/core/bbox/box_torch_ops.py:248-277 (rotate_nms_pcdet -> iou3d_nms_cuda.nms_gpu) and of
// det3d/core/utils/circle_nms_jit.py, and the decode of det3d/models/bbox_heads/center_head.py:342-419, 459-471.
//
// Boxes are taken as dal3_iou.hip takes them, [x, y, z, l, w, h, yaw] with l along the yaw. rotate_nms_pcdet first
// converts its boxes to pcdet's convention (columns 3 / 4 swapped, yaw -> -yaw - pi/2, box_torch_ops.py:255-257). That
// is NOT an isometry applied to the pair: the centres stay where they are while the rectangles turn from yaw to -yaw,
// so it changes the IoUs (on tests/nms_ref.py's clustered scene by up to 0.33, 53 pairs change sides of 0.7). It is
// therefore applied, on request (args.mirror), when a box is loaded: the IoU is then the bits of
// dal3_box_iou_pairwise on the converted boxes, and the reference's result is reproduced.
//
// NMS is two launches, each one workgroup per segment (a (frame, task) pair), whatever the grid:
//   sort      a stable least-significant-digit radix sort of the segment's (key, row) pairs, 8 bits a pass, key =
//             ~orderable(score) with every NaN mapped to 0 (first) and -0 to +0. It is the histogram -> scan ->
//             ballot-rank scatter of dal3_block.h's chunked sort with the segment as the one chunk and the histogram
//             in LDS (its own kernel, on the shared radix_tile_step): equal digits keep their input order, so equal
//             scores end by ascending row. Then the candidates' IouBox (sin / cos once per box) are written in sorted
//             order to the workspace: the one table the scan reads. It is O(K); no mask exists.
//   suppress  walks the candidates in blocks of 64, lane = candidate. (1) The block's 64 boxes are tested against the
//             boxes KEPT so far, the kept list split over the waves (each kept box is one broadcast load); a wave stops
//             when all its lanes are suppressed. (2) The block's own 64 x 64 triangle: wave w takes rows w, w + 4, ...,
//             one ballot per row = that row's 64 bits. (3) Every thread resolves the block from those 64 words in order
//             (bit i clear -> keep i, OR row i in). Only rows of kept boxes are ever evaluated against later columns
//             (the reference's n x n / 64 mask is read at kept rows only: typically a few hundred of 4096), and the
//             scan stops at post_max keeps, which cannot change the result.
// Every position is a function of the segment alone: no result depends on the grid or on the order atomics arrive in.
//
// The decode is an ordered compaction in three launches: per chunk of DEC_CHUNK cells the number of survivors, one
// exclusive scan per sample, then each chunk again with ballot ranks. A cell's mask and values come from one function
// (cell_eval) in both passes. The count and fill kernels are instantiated twice on the cell's evaluator: one view
// (dal3_center_decode) and the four flipped views of test_cfg.double_flip merged as they are read (dal3_center_decode_flip4,
// center_head.py:318-414: no un-flipped or merged map is written); scan, ranks and workspace are the same code.
#include "dal3_block.h"
#include "dal3_kernels.h"

// no FMA contraction: the IoU must be the bits of dal3_iou.hip's kernels (dal3_iou_pair.h), and the decode restates
// torch's float32 operations one by one
#pragma clang fp contract(off)

namespace {

constexpr int NMS_BLOCK = 256;
constexpr int NMS_WAVES = NMS_BLOCK / 64;
constexpr int DEC_BLOCK = 256;
constexpr int DEC_WAVES = DEC_BLOCK / 64;
constexpr int DEC_TILES = 4;
constexpr int64_t DEC_CHUNK = (int64_t)DEC_BLOCK * DEC_TILES;    // 1024 cells

#include "dal3_iou_pair.h"

struct NmsWs {
    uint32_t* key[2];                           // (K) each: the sort keys, ping-pong
    int32_t* idx[2];                            // (K) each: the rows (relative to the segment), ping-pong; [0] ends sorted
    int32_t* kept;                              // (K) the kept candidates' sorted positions, per segment at its rows
    void* table;                                // (K) IouBox<T> in sorted order
};

inline NmsWs carve_nms(Carver& c, int64_t K, int f64) {
    NmsWs w;
    for (int i = 0; i < 2; ++i) w.key[i] = c.take<uint32_t>((size_t)K);
    for (int i = 0; i < 2; ++i) w.idx[i] = c.take<int32_t>((size_t)K);
    w.kept = c.take<int32_t>((size_t)K);
    if (f64) w.table = c.take<IouBox<double>>((size_t)K);
    else w.table = c.take<IouBox<float>>((size_t)K);
    return w;
}

// ascending key = descending score; NaN first, -0 with +0
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 0u;
    uint32_t u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? u : (~u & 0x7fffffffu);
}

// the segment's rows [d0, d0 + n) and its candidates m; a segment that cannot be processed gives n = m = 0 and sets
// its status bit (every kernel decides alike)
__device__ __forceinline__ void nms_segment(const dal3_nms_args& a, int64_t f, int64_t& d0, int64_t& n, int64_t& m) {
    d0 = a.seg_offsets[f];
    const int64_t d1 = a.seg_offsets[f + 1];
    n = m = 0;
    if (d0 < 0 || d1 < d0 || d1 > a.K) {
        if (threadIdx.x == 0) atomicOr(a.status, DAL3_NMS_BAD_SEGMENT);
        d0 = 0;
        return;
    }
    int64_t rows = d1 - d0;
    if (a.seg_count) {
        const int64_t c = a.seg_count[f];
        rows = c < 0 ? 0 : (c < rows ? c : rows);
    }
    const int64_t cand = a.pre_max > 0 && a.pre_max < rows ? a.pre_max : rows;
    if (cand > DAL3_NMS_MAX_PRE) {
        if (threadIdx.x == 0) atomicOr(a.status, DAL3_NMS_TOO_MANY);
        return;
    }
    n = rows;
    m = cand;
}

template <typename T>
__device__ __forceinline__ IouBox<T> nms_box(const T* p, int yaw_col, int mirror) {
    T v[7] = {p[0], p[1], p[2], p[3], p[4], p[5], p[yaw_col]};
    if (mirror) {                               // box_torch_ops.py:255-257, in the input precision
        const T w = v[3];
        v[3] = v[4];
        v[4] = w;
        v[6] = -v[6] - (T)1.5707963267948966;
    }
    return iou_box(v);
}

template <typename T>
__global__ __launch_bounds__(NMS_BLOCK) void nms_sort_kernel(const dal3_nms_args a, const NmsWs ws) {
    __shared__ int32_t s_base[256];             // where the segment's next entry of each digit goes
    __shared__ int32_t s_scan[256];
    __shared__ int32_t s_wave[NMS_WAVES][256];  // the tile's count of each digit, per wave
    const int t = threadIdx.x;
    for (int64_t f = blockIdx.x; f < a.F; f += gridDim.x) {
        int64_t d0, n, m;
        nms_segment(a, f, d0, n, m);
        if (n == 0) continue;                   // uniform: no barrier is skipped by a part of the workgroup
        for (int64_t i = t; i < n; i += NMS_BLOCK) {
            ws.key[0][d0 + i] = score_key(a.scores[d0 + i]);
            ws.idx[0][d0 + i] = (int32_t)i;
        }
        __syncthreads();
        for (int pass = 0; pass < 4; ++pass) {
            const uint32_t* key_in = ws.key[pass & 1] + d0;
            const int32_t* idx_in = ws.idx[pass & 1] + d0;
            uint32_t* key_out = ws.key[(pass & 1) ^ 1] + d0;
            int32_t* idx_out = ws.idx[(pass & 1) ^ 1] + d0;
            const int shift = 8 * pass;
            s_base[t] = 0;
            __syncthreads();
            for (int64_t i = t; i < n; i += NMS_BLOCK) atomicAdd(&s_base[(key_in[i] >> shift) & 255], 1);
            __syncthreads();
            // exclusive scan of the 256 counts
            const int32_t mine = s_base[t];
            s_scan[t] = mine;
            __syncthreads();
            block_scan_inclusive<256>(s_scan);
            s_base[t] = s_scan[t] - mine;
            for (int64_t e0 = 0; e0 < n; e0 += NMS_BLOCK) {
                const int64_t i = e0 + t;
                const bool live = i < n;
                const uint32_t k = live ? key_in[i] : 0u;
                const int64_t o = radix_tile_step<NMS_WAVES>(live, (k >> shift) & 255, s_base, s_wave);
                if (o >= 0 && o < n) {          // live; the bound always holds for counts made from these keys
                    key_out[o] = k;
                    idx_out[o] = idx_in[i];
                }
            }
            __syncthreads();                    // the pass's stores are visible to the whole workgroup
        }
        // four passes: the sorted pairs are back in buffer 0
        const int32_t* idx = ws.idx[0] + d0;
        IouBox<T>* table = static_cast<IouBox<T>*>(ws.table) + d0;
        const T* boxes = static_cast<const T*>(a.boxes);
        for (int64_t c = t; c < n; c += NMS_BLOCK) {
            int64_t r = idx[c];
            if (r < 0 || r >= n) r = 0;         // cannot happen for a completed sort
            if (a.order) a.order[d0 + c] = (int32_t)r;
            if (c < m) table[c] = nms_box(boxes + (d0 + r) * a.box_stride, a.yaw_col, a.mirror);
        }
        __syncthreads();
    }
}

template <typename T, int MODE>
__device__ __forceinline__ bool suppresses(const IouBox<T>& i, const IouBox<T>& j, float thresh) {
    if (MODE == DAL3_NMS_CIRCLE) {
        const float dx = (float)(i.cx - j.cx), dy = (float)(i.cy - j.cy);
        const float xx = dx * dx, yy = dy * dy;
        return xx + yy <= thresh;
    }
    float bev, v3;
    box_iou_pair(i, j, bev, v3);
    return bev > thresh;
}

template <typename T, int MODE>
__global__ __launch_bounds__(NMS_BLOCK) void nms_suppress_kernel(const dal3_nms_args a, const NmsWs ws) {
    __shared__ unsigned long long s_rem[NMS_WAVES];     // the block's columns suppressed by earlier kept boxes, per wave
    __shared__ unsigned long long s_diag[64];           // row i of the block's own triangle
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int64_t f = blockIdx.x; f < a.F; f += gridDim.x) {
        int64_t d0, n, m;
        nms_segment(a, f, d0, n, m);
        const IouBox<T>* table = static_cast<const IouBox<T>*>(ws.table) + d0;
        const int32_t* idx = ws.idx[0] + d0;
        int32_t* kept = ws.kept + d0;
        int32_t* keep = a.keep + f * a.stride;
        int64_t limit = a.post_max > 0 && a.post_max < m ? a.post_max : m;
        if (limit > a.stride) limit = a.stride;         // the entry checked stride against the host offsets
        int64_t nk = 0;
        for (int64_t b0 = 0; b0 < m && nk < limit; b0 += 64) {
            const int cnt = (int)(m - b0 < 64 ? m - b0 : 64);
            const bool valid = lane < cnt;
            const IouBox<T> bj = table[valid ? b0 + lane : b0];
            // (1) against the boxes kept so far
            bool sup = false;
            for (int64_t k = wave; k < nk; k += NMS_WAVES) {
                const IouBox<T> ai = table[kept[k]];
                if (!sup) sup = suppresses<T, MODE>(ai, bj, a.thresh);
                if (__all(sup || !valid)) break;
            }
            const unsigned long long rem_w = __ballot(sup && valid);
            if (lane == 0) s_rem[wave] = rem_w;
            // (2) the block's own triangle
            for (int i = wave; i < cnt; i += NMS_WAVES) {
                const IouBox<T> ai = table[b0 + i];
                const bool bit = valid && lane > i && suppresses<T, MODE>(ai, bj, a.thresh);
                const unsigned long long row = __ballot(bit);
                if (lane == 0) s_diag[i] = row;
            }
            __syncthreads();
            // (3) in order
            unsigned long long rem = 0ull, keepbits = 0ull;
#pragma unroll
            for (int w = 0; w < NMS_WAVES; ++w) rem |= s_rem[w];
            for (int i = 0; i < cnt; ++i) {
                if (!((rem >> i) & 1ull)) {
                    keepbits |= 1ull << i;
                    rem |= s_diag[i];
                }
            }
            if (wave == 0 && ((keepbits >> lane) & 1ull)) {
                const int64_t p = nk + __popcll(keepbits & ((1ull << lane) - 1ull));
                if (p < limit) {
                    kept[p] = (int32_t)(b0 + lane);
                    keep[p] = idx[b0 + lane];
                }
            }
            nk += __popcll(keepbits);
            if (nk > limit) nk = limit;
            __syncthreads();                    // the kept list is visible; s_rem / s_diag are free again
        }
        if (t == 0) a.keep_count[f] = (int32_t)nk;
    }
}

// ---------------------------------------------------------------------------------- decode
__device__ __forceinline__ float map_at(const dal3_map& mp, int64_t b, int64_t row, int64_t col, int c) {
    return mp.data[b * mp.stride_b + row * mp.stride_h + col * mp.stride_w + c * mp.stride_c];
}

// The maps of one output cell. V = 1: the cell itself in sample b (dal3_center_decode). V = 4: the four views of merged
// sample b (dal3_center_decode_flip4), view v in map 4 b + v at the mirrored cell: rows reversed for v & 1 (y = -y), columns
// for v & 2 (x = -x). A reversed row or column is still a run of neighbouring addresses across the wave.
template <int V>
struct Views {
    int64_t b, row[2], col[2];                  // [0] as it is, [1] mirrored (V = 4 only)
    __device__ __forceinline__ Views(const dal3_center_decode_args& a, int64_t b_, int64_t r, int64_t c) : b(b_) {
        row[0] = r;
        col[0] = c;
        row[1] = a.H - 1 - r;
        col[1] = a.W - 1 - c;
    }
    // view v's value of channel c
    __device__ __forceinline__ float at(const dal3_map& mp, int v, int c) const {
        return map_at(mp, V * b + v, row[v & 1], col[(v >> 1) & 1], c);
    }
};

// torch.mean(dim=1) over the four views on the CPU: a running sum in view order, then one division
__device__ __forceinline__ float mean4(float a0, float a1, float a2, float a3) { return (((a0 + a1) + a2) + a3) / 4.f; }

// channel c of a two-channel map after the un-flip of its values, merged: channel 0 belongs to x and changes under the
// x-flips (views 2, 3), channel 1 to y and changes under the y-flips (views 1, 3). ONE_MINUS: reg (1 - r), else rot / vel (-r).
template <int V, bool ONE_MINUS>
__device__ __forceinline__ float merged_xy(const Views<V>& w, const dal3_map& mp, int c) {
    if constexpr (V == 1) {
        return w.at(mp, 0, c);
    } else {
        float r[4];
        for (int v = 0; v < 4; ++v) {
            const float x = w.at(mp, v, c);
            const bool flipped = c == 0 ? (v & 2) != 0 : (v & 1) != 0;
            r[v] = !flipped ? x : ONE_MINUS ? 1.f - x : -x;
        }
        return mean4(r[0], r[1], r[2], r[3]);
    }
}

// a channel no flip changes (height), merged
template <int V>
__device__ __forceinline__ float merged(const Views<V>& w, const dal3_map& mp, int c) {
    if constexpr (V == 1) return w.at(mp, 0, c);
    else return mean4(w.at(mp, 0, c), w.at(mp, 1, c), w.at(mp, 2, c), w.at(mp, 3, c));
}

__device__ __forceinline__ float sigmoid_of(float h) {
    const float e = expf(-h);
    return 1.f / (1.f + e);
}

struct Cell {
    float x, y, z, score;
    int32_t label;
};

// post_processing's mask of one cell and the values it is taken on (center_head.py:342-362, 397-401, 459-465)
template <int V>
__device__ __forceinline__ bool cell_eval(const dal3_center_decode_args& a, const Views<V>& w, int64_t row, int64_t col,
                                          Cell& o) {
    float best = 0.f;
    int32_t label = 0;
    for (int c = 0; c < a.C; ++c) {
        float s;
        if constexpr (V == 1) s = sigmoid_of(w.at(a.hm, 0, c));
        else
            s = mean4(sigmoid_of(w.at(a.hm, 0, c)), sigmoid_of(w.at(a.hm, 1, c)), sigmoid_of(w.at(a.hm, 2, c)),
                      sigmoid_of(w.at(a.hm, 3, c)));
        // torch.max: the first maximum, a NaN wins and stays
        if (c == 0 || (best == best && (s > best || s != s))) {
            best = s;
            label = c;
        }
    }
    o.score = best;
    o.label = label;
    const float fx = (float)col + merged_xy<V, true>(w, a.reg, 0);
    const float fy = (float)row + merged_xy<V, true>(w, a.reg, 1);
    const float sx = fx * a.out_size_factor, sy = fy * a.out_size_factor;
    const float vx = sx * a.voxel_size[0], vy = sy * a.voxel_size[1];
    o.x = vx + a.pc_range[0];
    o.y = vy + a.pc_range[1];
    o.z = merged<V>(w, a.height, 0);
    bool ok = best > a.score_threshold;
    if (a.has_range)
        ok = ok && o.x >= a.range[0] && o.y >= a.range[1] && o.z >= a.range[2] && o.x <= a.range[3] && o.y <= a.range[4] &&
             o.z <= a.range[5];
    return ok;
}

// the columns of a survivor's row that the mask does not need: dim, vel, rot (center_head.py:344, 364-382, 403-414)
template <int V>
__device__ __forceinline__ void cell_rest(const dal3_center_decode_args& a, const Views<V>& w, float* q, int cols) {
    for (int j = 0; j < 3; ++j) {
        if constexpr (V == 1) q[3 + j] = expf(w.at(a.dim, 0, j));
        else q[3 + j] = mean4(expf(w.at(a.dim, 0, j)), expf(w.at(a.dim, 1, j)), expf(w.at(a.dim, 2, j)), expf(w.at(a.dim, 3, j)));
    }
    if (a.vel.data) {
        q[6] = merged_xy<V, false>(w, a.vel, 0);
        q[7] = merged_xy<V, false>(w, a.vel, 1);
    }
    q[cols - 1] = atan2f(merged_xy<V, false>(w, a.rot, 0), merged_xy<V, false>(w, a.rot, 1));
}

template <int V>
__global__ __launch_bounds__(DEC_BLOCK) void decode_count_kernel(const dal3_center_decode_args a, int32_t* counts,
                                                                 int64_t chunks) {
    __shared__ int32_t s_cnt;
    const int64_t HW = a.H * a.W;
    for (int64_t job = blockIdx.x; job < a.B * chunks; job += gridDim.x) {
        const int64_t b = job / chunks, c = job - b * chunks;
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        int32_t mine = 0;
        for (int r = 0; r < DEC_TILES; ++r) {
            const int64_t cell = c * DEC_CHUNK + (int64_t)r * DEC_BLOCK + threadIdx.x;
            Cell o;
            const uint32_t row = (uint32_t)cell / (uint32_t)a.W, col = (uint32_t)cell - row * (uint32_t)a.W;   // H W <= 2^24
            const bool ok = cell < HW && cell_eval<V>(a, Views<V>(a, b, row, col), row, col, o);
            mine += __popcll(__ballot(ok));
        }
        if ((threadIdx.x & 63) == 0) atomicAdd(&s_cnt, mine);   // integers: the order does not matter
        __syncthreads();
        if (threadIdx.x == 0) counts[job] = s_cnt;
        __syncthreads();
    }
}

// per sample: the exclusive scan of its chunks' counts in place, and the segment's count
__global__ __launch_bounds__(DEC_BLOCK) void decode_scan_kernel(const dal3_center_decode_args a, int32_t* counts,
                                                                int64_t chunks) {
    __shared__ int64_t s_part[DEC_BLOCK];
    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int64_t total = block_scan_spans<DEC_BLOCK>(counts + b * chunks, chunks, s_part);
        if (threadIdx.x == DEC_BLOCK - 1) {
            const int64_t f = a.seg_first + b * a.seg_step;
            const int64_t d0 = a.seg_offsets[f], d1 = a.seg_offsets[f + 1];
            int64_t cap = d1 - d0;
            if (d0 < 0 || d1 < d0 || d1 > a.K) {
                atomicOr(a.status, DAL3_NMS_BAD_SEGMENT);
                cap = 0;
            } else if (total > cap) {
                atomicOr(a.status, DAL3_DECODE_OVERFLOW);
            }
            a.seg_count[f] = (int32_t)(total < cap ? total : cap);
        }
        __syncthreads();
    }
}

template <int V>
__global__ __launch_bounds__(DEC_BLOCK) void decode_fill_kernel(const dal3_center_decode_args a, const int32_t* counts,
                                                                int64_t chunks) {
    __shared__ int32_t s_wave[DEC_WAVES];
    const int t = threadIdx.x;
    const int64_t HW = a.H * a.W;
    const int cols = a.vel.data ? 9 : 7;
    for (int64_t job = blockIdx.x; job < a.B * chunks; job += gridDim.x) {
        const int64_t b = job / chunks, c = job - b * chunks;
        const int64_t f = a.seg_first + b * a.seg_step;
        const int64_t d0 = a.seg_offsets[f], d1 = a.seg_offsets[f + 1];
        const int64_t cap = d0 < 0 || d1 < d0 || d1 > a.K ? 0 : d1 - d0;
        int64_t base = counts[job];
        for (int r = 0; r < DEC_TILES; ++r) {
            const int64_t cell = c * DEC_CHUNK + (int64_t)r * DEC_BLOCK + t;
            const uint32_t row = (uint32_t)cell / (uint32_t)a.W, col = (uint32_t)cell - row * (uint32_t)a.W;
            Cell o;
            const Views<V> w(a, b, row, col);
            const bool ok = cell < HW && cell_eval<V>(a, w, row, col, o);
            int32_t tile;
            const int64_t pos = base + block_rank<DEC_WAVES>(ok, s_wave, tile);
            if (ok && pos >= 0 && pos < cap) {
                const int64_t k = d0 + pos;
                float* q = a.boxes + k * cols;
                q[0] = o.x;
                q[1] = o.y;
                q[2] = o.z;
                cell_rest<V>(a, w, q, cols);
                a.scores[k] = o.score;
                a.labels[k] = o.label;
                a.cell[k] = (int32_t)cell;
            }
            base += tile;
        }
    }
}

// ---------------------------------------------------------------------------------- DoubleFlip's points
constexpr int FLIP_BLOCK = 256;

// one thread per input element: read once, written to the sample's four views; then out_offsets
__global__ __launch_bounds__(FLIP_BLOCK) void flip4_points_kernel(const uint32_t* __restrict__ points, int64_t N, int C,
                                                                  const int64_t* __restrict__ offsets, int64_t B,
                                                                  uint32_t* __restrict__ out, int64_t* __restrict__ out_offsets) {
    const int64_t stride = (int64_t)gridDim.x * FLIP_BLOCK, first = (int64_t)blockIdx.x * FLIP_BLOCK + threadIdx.x;
    for (int64_t i = first; i < N * C; i += stride) {
        const int64_t r = i / C;
        const int c = (int)(i - r * C);
        // the sample of row r: the last b with offsets[b] <= r
        int64_t lo = 0, hi = B;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (offsets[mid] <= r) lo = mid;
            else hi = mid;
        }
        const int64_t o0 = offsets[lo], o1 = offsets[lo + 1];
        if (r < o0 || r >= o1) continue;        // a row of no sample
        const int64_t n = o1 - o0;
        const uint32_t x = points[i];
        for (int v = 0; v < 4; ++v) {
            const int64_t row = 4 * o0 + v * n + (r - o0);
            if (row < 0 || row >= 4 * N) continue;   // only offsets that are no CSR of [0, N] get here
            const bool neg = (c == 0 && (v & 2)) || (c == 1 && (v & 1));
            out[row * C + c] = neg ? x ^ 0x80000000u : x;
        }
    }
    for (int64_t j = first; j <= 4 * B; j += stride) {
        const int64_t b = j >> 2, v = j & 3;
        out_offsets[j] = b == B ? 4 * offsets[B] : 4 * offsets[b] + v * (offsets[b + 1] - offsets[b]);
    }
}

}  // namespace

size_t nms_workspace_bytes(int64_t K, int boxes_f64) {
    Carver c(nullptr, 0);
    carve_nms(c, K, boxes_f64);
    return c.off;
}

hipError_t launch_nms(const dal3_nms_args* args, hipStream_t s) {
    const dal3_nms_args& a = *args;
    if (a.F <= 0) return hipSuccess;
    Carver c(a.workspace, a.workspace_bytes);
    const NmsWs ws = carve_nms(c, a.K, a.boxes_f64);
    const dim3 g(grid_clamp(a.F, GRID_MAX, a.max_workgroups)), blk(NMS_BLOCK);
    if (a.K > 0) {
        if (a.boxes_f64) hipLaunchKernelGGL(nms_sort_kernel<double>, g, blk, 0, s, a, ws);
        else hipLaunchKernelGGL(nms_sort_kernel<float>, g, blk, 0, s, a, ws);
    }
    if (a.boxes_f64) {
        if (a.mode == DAL3_NMS_CIRCLE) hipLaunchKernelGGL((nms_suppress_kernel<double, DAL3_NMS_CIRCLE>), g, blk, 0, s, a, ws);
        else hipLaunchKernelGGL((nms_suppress_kernel<double, DAL3_NMS_ROTATE>), g, blk, 0, s, a, ws);
    } else {
        if (a.mode == DAL3_NMS_CIRCLE) hipLaunchKernelGGL((nms_suppress_kernel<float, DAL3_NMS_CIRCLE>), g, blk, 0, s, a, ws);
        else hipLaunchKernelGGL((nms_suppress_kernel<float, DAL3_NMS_ROTATE>), g, blk, 0, s, a, ws);
    }
    return hipGetLastError();
}

static int64_t decode_chunks(int64_t H, int64_t W) { return (H * W + DEC_CHUNK - 1) / DEC_CHUNK; }

// the one array: every (sample, chunk)'s survivors, then their exclusive scan per sample
static int32_t* carve_decode(Carver& c, int64_t B, int64_t H, int64_t W) {
    return c.take<int32_t>((size_t)(B * decode_chunks(H, W)));
}

size_t center_decode_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    Carver c(nullptr, 0);
    carve_decode(c, B, H, W);
    return c.off;
}

template <int V>
static hipError_t launch_decode(const dal3_center_decode_args& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    const int64_t chunks = decode_chunks(a.H, a.W);
    Carver c(a.workspace, a.workspace_bytes);
    int32_t* counts = carve_decode(c, a.B, a.H, a.W);
    const dim3 jobs(grid_clamp(a.B * chunks, GRID_MAX, a.max_workgroups)), samples(grid_clamp(a.B, GRID_MAX, a.max_workgroups));
    if (chunks > 0) hipLaunchKernelGGL(decode_count_kernel<V>, jobs, dim3(DEC_BLOCK), 0, s, a, counts, chunks);
    hipLaunchKernelGGL(decode_scan_kernel, samples, dim3(DEC_BLOCK), 0, s, a, counts, chunks);
    if (chunks > 0) hipLaunchKernelGGL(decode_fill_kernel<V>, jobs, dim3(DEC_BLOCK), 0, s, a, counts, chunks);
    return hipGetLastError();
}

hipError_t launch_center_decode(const dal3_center_decode_args* args, hipStream_t s) { return launch_decode<1>(*args, s); }

// the merged samples' chunks: the same array, scan and ranks as the one-view decode
hipError_t launch_center_decode_flip4(const dal3_center_decode_flip4_args* args, hipStream_t s) {
    return launch_decode<4>(args->decode, s);
}

hipError_t launch_flip4_points(const float* points, int64_t N, int C, const int64_t* offsets, int64_t B, float* out,
                               int64_t* out_offsets, int64_t max_workgroups, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    const int64_t work = N * C > 4 * B + 1 ? N * C : 4 * B + 1;
    const unsigned grid = grid_clamp((work + FLIP_BLOCK - 1) / FLIP_BLOCK, 65536, max_workgroups);
    hipLaunchKernelGGL(flip4_points_kernel, dim3(grid), dim3(FLIP_BLOCK), 0, s,
                       reinterpret_cast<const uint32_t*>(points), N, C, offsets, B, reinterpret_cast<uint32_t*>(out),
                       out_offsets);
    return hipGetLastError();
}
