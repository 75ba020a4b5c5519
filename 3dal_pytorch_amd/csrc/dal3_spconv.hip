// dal3_spconv.hip — the sparse 3-D middle of the VoxelNet detector (dal3_sp_* of include/dal3.h): the site bookkeeping
// and the convolutions of SpMiddleResNetFHD (det3d/models/backbones/scn.py), which the reference delegates to spconv 1.x.
//
// Bookkeeping (integers only). A site is the 32-bit key ((b * D + z) * H + y) * W + x; a row that is no site (beyond the
// device count, or outside the grid) gets the key B * D * H * W, behind every real one.
//   sort        dal3_block.h's chunked radix sort of (key, row) pairs: the sorted keys and their rows are what every
//               neighbour table of the level searches (lower_bound). Equal neighbouring keys are duplicates.
//   downsample  every input site writes the keys of the output sites whose receptive field holds it (at most
//               ceil(k / s) per axis), the candidates are sorted, the head of each run of equal keys is an output
//               site, and the exclusive scan of the head flags in sorted order (per 256-entry tile: count, scan of the
//               counts, ballot ranks) is its row: the output rows ascend by key.
//   table       (taps, capacity) int32, tap-major: row of the input site under tap k of output site i, or -1; a wave's
//               32 sites read consecutive words. tap = (kz * KH + ky) * KW + kx, the weight's own order.
// No atomic decides a position or a count, every loop is a grid-stride loop over elements: the bytes do not depend on the
// grid.
//
// The convolution is one output-stationary gather-GEMM body on v_mfma_f32_32x32x2_f32 in the orientation of
// dal3_device.h: output channels on the MFMA rows, 32 output sites on its columns (= lanes). A wave owns a tile of 32
// sites and MTW tiles of 32 output channels. Per tap a lane reads its site's neighbour row from the table and gathers
// that row's channels from global memory: lane half h owns the contiguous channels [h * CP / 2, (h + 1) * CP / 2) of the
// zero-padded CP input channels, so k-step s pairs channel s with channel CP / 2 + s and the gather is dwordx4 loads of
// one row (scalar loads for the 1 .. 8 channels of the first layer). An absent neighbour supplies zeros; a tap that no
// site of the tile has is skipped wave-uniformly. A tap's products are summed from zero and then added to the total, taps
// in ascending order: the sum's order is fixed by the site's row alone. The weights come fragment-packed in consumption
// order [tap][4 k-steps][out tile][lane] float4 behind a flag word and the folded bias. The epilogue adds the residual
// row, applies the ReLU (a NaN stays a NaN) and stores the row, or scatters it into channel c * D + d of a BEV canvas.
#include "dal3_block.h"
#include "dal3_kernels.h"

namespace {

constexpr int SP_BLOCK = 256, SP_WAVES = SP_BLOCK / 64;
constexpr int SP_HEAD_FLOATS = 64;              // the pack's first section: word 0 is its flag

inline unsigned sp_grid(int64_t want, int64_t max_workgroups) { return grid_clamp(want, 65535 * 16, max_workgroups); }
__host__ __device__ inline int64_t sp_tiles(int64_t n) { return (n + SP_BLOCK - 1) / SP_BLOCK; }

// rows in use: the device count clamped to the capacity; without a count every row
__device__ __forceinline__ int64_t sp_live(const int64_t* n, int64_t cap) {
    if (!n) return cap;
    const int64_t v = *n;
    return v < 0 ? 0 : v > cap ? cap : v;
}

struct SpShape {
    int32_t B, D, H, W;
};

// the key of row i of an (n, 4) [b, z, y, x] table, -1 when the row is outside the grid
__device__ __forceinline__ int32_t sp_key_of(const int32_t* idx, int64_t i, const SpShape& g) {
    const int32_t b = idx[4 * i], z = idx[4 * i + 1], y = idx[4 * i + 2], x = idx[4 * i + 3];
    if (b < 0 || b >= g.B || z < 0 || z >= g.D || y < 0 || y >= g.H || x < 0 || x >= g.W) return -1;
    return (int32_t)((((int64_t)b * g.D + z) * g.H + y) * g.W + x);
}

__global__ __launch_bounds__(SP_BLOCK) void sp_keys_kernel(const int32_t* idx, int64_t cap, const int64_t* n_ptr, SpShape g,
                                                           int32_t none, int32_t* key, int32_t* status) {
    const int64_t n = sp_live(n_ptr, cap);
    for (int64_t i = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; i < cap; i += (int64_t)gridDim.x * SP_BLOCK) {
        int32_t k = none;
        if (i < n) {
            const int32_t v = sp_key_of(idx, i, g);
            if (v >= 0) k = v;
            else atomicOr(status, DAL3_SP_BAD_COORD);
        }
        key[i] = k;
    }
}

__global__ __launch_bounds__(SP_BLOCK) void sp_sorted_kernel(const int32_t* key, const int32_t* pos, int64_t cap, int32_t none,
                                                             int32_t* out_key, int32_t* out_pos, int32_t* status) {
    for (int64_t r = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; r < cap; r += (int64_t)gridDim.x * SP_BLOCK) {
        const int32_t k = key[r];
        out_key[r] = k;
        out_pos[r] = pos[r];
        if (k < none && r + 1 < cap && key[r + 1] == k) atomicOr(status, DAL3_SP_DUPLICATE);
    }
}

struct SpWindow {
    int32_t k[3], s[3], p[3];
};

// candidate c of input row i: per axis the j-th output coordinate whose window holds the input coordinate
__global__ __launch_bounds__(SP_BLOCK) void sp_candidates_kernel(const int32_t* idx, int64_t cap, const int64_t* n_ptr, SpShape in,
                                                                 SpShape out, SpWindow w, int nz, int ny, int nx, int32_t none,
                                                                 int32_t* key) {
    const int64_t n = sp_live(n_ptr, cap), cand = (int64_t)nz * ny * nx, E = cap * cand;
    for (int64_t e = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; e < E; e += (int64_t)gridDim.x * SP_BLOCK) {
        const int64_t i = e / cand;
        const int c = (int)(e % cand);
        int32_t k = none;
        if (i < n && sp_key_of(idx, i, in) >= 0) {
            const int j[3] = {c / (ny * nx), (c / nx) % ny, c % nx};
            const int32_t ext[3] = {out.D, out.H, out.W};
            int32_t o[3];
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int32_t t = idx[4 * i + 1 + a] + w.p[a];      // o * s <= t < o * s + k
                o[a] = t / w.s[a] - j[a];
                if (o[a] < 0 || o[a] >= ext[a] || t - o[a] * w.s[a] >= w.k[a]) ok = false;
            }
            if (ok) k = (int32_t)((((int64_t)idx[4 * i] * out.D + o[0]) * out.H + o[1]) * out.W + o[2]);
        }
        key[e] = k;
    }
}

__device__ __forceinline__ bool sp_head(const int32_t* key, int64_t r, int64_t E, int32_t none) {
    return r < E && key[r] < none && (r == 0 || key[r - 1] != key[r]);
}

__global__ __launch_bounds__(SP_BLOCK) void sp_head_count_kernel(const int32_t* key, int64_t E, int32_t none, int32_t* tile) {
    __shared__ int32_t s_cnt[SP_WAVES];
    const int64_t tiles = sp_tiles(E);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        int32_t total;
        block_rank<SP_WAVES>(sp_head(key, t * SP_BLOCK + threadIdx.x, E, none), s_cnt, total);
        if (threadIdx.x == 0) tile[t] = total;
    }
}

// tile: scanned. The head of rank r is output site r: its coordinates and key; ranks beyond the capacity set the bit
__global__ __launch_bounds__(SP_BLOCK) void sp_emit_kernel(const int32_t* key, int64_t E, int32_t none, const int32_t* tile,
                                                           const int64_t* total, SpShape out, int64_t out_cap, int32_t* out_idx,
                                                           int32_t* out_key, int64_t* n_out, int32_t* status) {
    __shared__ int32_t s_cnt[SP_WAVES];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t n = *total;
        *n_out = n > out_cap ? out_cap : n;
    }
    const int64_t tiles = sp_tiles(E);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r = t * SP_BLOCK + threadIdx.x;
        const bool head = sp_head(key, r, E, none);
        int32_t cnt;
        const int64_t rank = (int64_t)tile[t] + block_rank<SP_WAVES>(head, s_cnt, cnt);
        if (!head) continue;
        if (rank >= out_cap) {
            atomicOr(status, DAL3_SP_OVERFLOW);
            continue;
        }
        const int32_t k = key[r];
        out_key[rank] = k;
        int32_t* o = out_idx + 4 * rank;
        o[3] = k % out.W;
        o[2] = (k / out.W) % out.H;
        o[1] = (int32_t)((k / ((int64_t)out.W * out.H)) % out.D);
        o[0] = (int32_t)(k / ((int64_t)out.W * out.H * out.D));
    }
}

// an empty level: no candidate was sorted
__global__ void sp_zero_count_kernel(int64_t* n_out) { *n_out = 0; }

__global__ __launch_bounds__(SP_BLOCK) void sp_table_kernel(const int32_t* out_idx, int64_t out_cap, const int64_t* n_out_ptr,
                                                            SpShape in, SpShape out, SpWindow w, const int32_t* in_key,
                                                            const int32_t* in_pos, int64_t in_cap, const int64_t* n_in_ptr,
                                                            int32_t* table) {
    const int64_t n_out = sp_live(n_out_ptr, out_cap), n_in = sp_live(n_in_ptr, in_cap);
    const int taps = w.k[0] * w.k[1] * w.k[2];
    const int64_t total = (int64_t)taps * out_cap;
    for (int64_t e = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * SP_BLOCK) {
        const int64_t i = e % out_cap;
        const int tap = (int)(e / out_cap);
        if (i >= n_out) continue;
        int32_t found = -1;
        if (sp_key_of(out_idx, i, out) >= 0) {
            const int kk[3] = {tap / (w.k[1] * w.k[2]), (tap / w.k[2]) % w.k[1], tap % w.k[2]};
            const int32_t ext[3] = {in.D, in.H, in.W};
            int32_t c[3];
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                c[a] = out_idx[4 * i + 1 + a] * w.s[a] - w.p[a] + kk[a];
                if (c[a] < 0 || c[a] >= ext[a]) ok = false;
            }
            if (ok) {
                const int32_t k = (int32_t)((((int64_t)out_idx[4 * i] * in.D + c[0]) * in.H + c[1]) * in.W + c[2]);
                const int64_t lo = lower_bound(in_key, 0, n_in, k);
                if (lo < n_in && in_key[lo] == k) {
                    const int64_t p = in_pos ? in_pos[lo] : lo;
                    if (p >= 0 && p < in_cap) found = (int32_t)p;
                }
            }
        }
        table[e] = found;
    }
}

// ---------------------------------------------------------------------------------- the convolution
__host__ __device__ constexpr int sp_cp(int c_in) { return c_in <= 8 ? 8 : c_in; }    // zero-padded input channels

// (the fold itself: dal3_fold.h; the layout, the non-finite flag and the 64-float head are this packer's own)
__global__ __launch_bounds__(SP_BLOCK) void sp_conv_pack_kernel(const FoldLayer L, int taps, int mt_total, int ns4, int64_t total,
                                                                float* out, int32_t* status) {
    const int half = sp_cp(L.c_in) / 2;
    for (int64_t i = SP_HEAD_FLOATS + (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SP_BLOCK) {
        float v = 0.f;
        const int64_t at = i - SP_HEAD_FLOATS;
        if (at < (int64_t)mt_total * 32) {
            const int co = (int)at;
            if (co < L.c_out) v = fold_bias(L, co);
        } else {
            const int64_t j = at - (int64_t)mt_total * 32;
            const int e = (int)(j & 3), lane = (int)((j >> 2) & 63);
            const int64_t t = j >> 8;
            const int mt = (int)(t % mt_total), s4 = (int)((t / mt_total) % ns4), tap = (int)(t / ((int64_t)mt_total * ns4));
            const int co = 32 * mt + (lane & 31), ci = (lane >> 5) * half + 4 * s4 + e;
            if (co < L.c_out && ci < L.c_in) v = fold_weight(L, ((int64_t)tap * L.c_in + ci) * L.c_out + co, co);
        }
        if (bits_nonfinite(v)) {
            atomicOr(reinterpret_cast<int32_t*>(out), 1);
            if (status) atomicOr(status, DAL3_SP_BAD_WEIGHT);
        }
        out[i] = v;
    }
}

struct SpConvGeom {
    int taps, c_in, c_out, relu, center, mt_total, n_groups, ns4;
    int64_t in_cap, out_cap, n_work;
    const int64_t* n_out;
    const int32_t* table;
    const float *x, *residual;
    float* y;
    const int32_t* flag;
    const float* bias;
    const f32x4* frag;
    float* canvas;
    const int32_t* out_idx;
    int32_t cB, cD, cH, cW;
    int32_t* status;
};

// max(v, 0) that keeps a NaN (torch.relu does) and turns -0 into +0
__device__ __forceinline__ float sp_relu(float v) { return v > 0.f ? v : (v == v ? 0.f : v); }

// CP: padded input channels (8: the first layer's 1 .. 8, scalar loads); MTW: out tiles of 32 channels per wave
template <int CP, int MTW>
__global__ __launch_bounds__(SP_BLOCK) void sp_conv_kernel(const SpConvGeom g) {
    constexpr int HALF = CP / 2, KC = HALF < 16 ? HALF : 16, NCH = HALF / KC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
    if (*g.flag) {                              // a folded weight is not finite: the pack is refused
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(g.status, DAL3_SP_BAD_WEIGHT);
        return;
    }
    const int64_t n_out = sp_live(g.n_out, g.out_cap);
    for (int64_t work = (int64_t)blockIdx.x * SP_WAVES + wave; work < g.n_work; work += (int64_t)gridDim.x * SP_WAVES) {
        const int grp = (int)(work % g.n_groups);
        const int64_t i0 = (work / g.n_groups) * 32;
        if (i0 >= n_out) continue;
        const int64_t i = i0 + n;
        const bool live = i < n_out;
        const int mt0 = grp * MTW;

        f32x16 acc[MTW];
#pragma unroll
        for (int m = 0; m < MTW; ++m) acc[m] = tile_from_channels(g.bias + 32 * (mt0 + m), h);

        for (int tap = 0; tap < g.taps; ++tap) {
            int32_t idx = live ? g.table[(int64_t)tap * g.out_cap + i] : -1;
            if (idx >= g.in_cap) idx = -1;
            if (__ballot(idx >= 0) == 0ull) continue;
            const float* row = g.x + (int64_t)(idx < 0 ? 0 : idx) * g.c_in;
            f32x16 part[MTW];
#pragma unroll
            for (int m = 0; m < MTW; ++m) part[m] = f32x16{};
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                float bv[KC];
                if (CP == 8) {
#pragma unroll
                    for (int s = 0; s < KC; ++s) {
                        const int c = h * HALF + s;
                        bv[s] = (idx >= 0 && c < g.c_in) ? row[c] : 0.f;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < KC / 4; ++q) {
                        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (idx >= 0) v = *reinterpret_cast<const f32x4*>(row + h * HALF + ch * KC + 4 * q);
                        bv[4 * q] = v[0], bv[4 * q + 1] = v[1], bv[4 * q + 2] = v[2], bv[4 * q + 3] = v[3];
                    }
                }
#pragma unroll
                for (int s4 = 0; s4 < KC / 4; ++s4) {
                    const int64_t at = (((int64_t)tap * g.ns4 + ch * (KC / 4) + s4) * g.mt_total + mt0) * 64 + lane;
                    f32x4 a[MTW];
#pragma unroll
                    for (int m = 0; m < MTW; ++m) a[m] = g.frag[at + 64 * m];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
#pragma unroll
                        for (int m = 0; m < MTW; ++m) part[m] = mfma32(a[m][e], bv[4 * s4 + e], part[m]);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < MTW; ++m) acc[m] += part[m];
        }

        if (!live) continue;
        // a row that is no site (its centre tap is absent: only a bad input row of a submanifold layer) is +0
        const bool zero = g.center >= 0 && g.table[(int64_t)g.center * g.out_cap + i] < 0;
        int32_t cb = 0, cz = 0, cy = 0, cx = 0;
        bool on_canvas = false;
        if (g.canvas) {
            cb = g.out_idx[4 * i], cz = g.out_idx[4 * i + 1], cy = g.out_idx[4 * i + 2], cx = g.out_idx[4 * i + 3];
            on_canvas = cb >= 0 && cb < g.cB && cz >= 0 && cz < g.cD && cy >= 0 && cy < g.cH && cx >= 0 && cx < g.cW;
        }
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c0 = 32 * (mt0 + m) + 8 * q + 4 * h;     // registers 4q .. 4q + 3: four consecutive channels
                if (c0 >= g.c_out) continue;
                f32x4 v = f32x4{acc[m][4 * q], acc[m][4 * q + 1], acc[m][4 * q + 2], acc[m][4 * q + 3]};
                if (g.residual) v += *reinterpret_cast<const f32x4*>(g.residual + i * g.c_out + c0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (g.relu) v[e] = sp_relu(v[e]);
                    if (zero) v[e] = 0.f;
                }
                if (g.y) *reinterpret_cast<f32x4*>(g.y + i * g.c_out + c0) = v;
                if (on_canvas) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        g.canvas[((((int64_t)cb * g.c_out + c0 + e) * g.cD + cz) * g.cH + cy) * g.cW + cx] = v[e];
                }
            }
        }
    }
}

template <int CP>
void sp_launch_cp(const SpConvGeom& g, int mtw, dim3 grid, hipStream_t s) {
    if (mtw == 2) hipLaunchKernelGGL((sp_conv_kernel<CP, 2>), grid, dim3(SP_BLOCK), 0, s, g);
    else hipLaunchKernelGGL((sp_conv_kernel<CP, 1>), grid, dim3(SP_BLOCK), 0, s, g);
}

inline SpShape sp_shape(int64_t B, const int32_t* s) { return {(int32_t)B, s[0], s[1], s[2]}; }
inline SpWindow sp_window(const int32_t* k, const int32_t* s, const int32_t* p) {
    return {{k[0], k[1], k[2]}, {s[0], s[1], s[2]}, {p[0], p[1], p[2]}};
}
inline int sp_axis_candidates(int k, int s) { return (k + s - 1) / s; }

struct SpDownWs {
    RadixBufs<int32_t> sort;
    int32_t* tile;
    int64_t* total;
};
inline SpDownWs carve_down(Carver& c, int64_t E) {
    SpDownWs w;
    w.sort = carve_radix<int32_t>(c, E, 2);
    w.tile = c.take<int32_t>((size_t)sp_tiles(E));
    w.total = c.take<int64_t>(1);
    return w;
}

}  // namespace

size_t sp_sort_workspace_bytes(int64_t capacity) {
    Carver c(nullptr, 0);
    carve_radix<int32_t>(c, capacity, 2);
    return c.off;
}

hipError_t launch_sp_sort(const dal3_sp_sort_args* args, hipStream_t s) {
    const dal3_sp_sort_args& a = *args;
    if (a.capacity <= 0) return hipSuccess;
    Carver c(a.workspace, a.workspace_bytes);
    const RadixBufs<int32_t> b = carve_radix<int32_t>(c, a.capacity, 2);
    const SpShape g = sp_shape(a.B, a.shape);
    const int64_t none = (int64_t)g.B * g.D * g.H * g.W;
    const int passes = radix_passes(none);
    const dim3 grid(sp_grid(sp_tiles(a.capacity), a.max_workgroups)), blk(SP_BLOCK);
    hipLaunchKernelGGL(sp_keys_kernel, grid, blk, 0, s, a.indices, a.capacity, a.n, g, (int32_t)none, b.key[0], a.status);
    const hipError_t e = radix_sort_pairs(b, a.capacity, passes, sp_grid(radix_chunks(a.capacity), a.max_workgroups), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sp_sorted_kernel, grid, blk, 0, s, b.key[passes & 1], b.pos[passes & 1], a.capacity, (int32_t)none,
                       a.sorted_key, a.sorted_pos, a.status);
    return hipGetLastError();
}

int sp_candidates(const int32_t* kernel, const int32_t* stride) {
    return sp_axis_candidates(kernel[0], stride[0]) * sp_axis_candidates(kernel[1], stride[1]) *
           sp_axis_candidates(kernel[2], stride[2]);
}

size_t sp_downsample_workspace_bytes(int64_t in_capacity, int candidates) {
    Carver c(nullptr, 0);
    carve_down(c, in_capacity * candidates);
    return c.off;
}

hipError_t launch_sp_downsample(const dal3_sp_downsample_args* args, hipStream_t s) {
    const dal3_sp_downsample_args& a = *args;
    const int nz = sp_axis_candidates(a.kernel[0], a.stride[0]), ny = sp_axis_candidates(a.kernel[1], a.stride[1]),
              nx = sp_axis_candidates(a.kernel[2], a.stride[2]);
    const int64_t E = a.in_capacity * nz * ny * nx;
    if (E <= 0) {
        hipLaunchKernelGGL(sp_zero_count_kernel, dim3(1), dim3(1), 0, s, a.n_out);
        return hipGetLastError();
    }
    Carver c(a.workspace, a.workspace_bytes);
    const SpDownWs w = carve_down(c, E);
    const SpShape in = sp_shape(a.B, a.in_shape), out = sp_shape(a.B, a.out_shape);
    const int64_t none = (int64_t)out.B * out.D * out.H * out.W;
    const int passes = radix_passes(none);
    const dim3 grid(sp_grid(sp_tiles(E), a.max_workgroups)), blk(SP_BLOCK);
    hipLaunchKernelGGL(sp_candidates_kernel, grid, blk, 0, s, a.in_indices, a.in_capacity, a.n_in, in, out,
                       sp_window(a.kernel, a.stride, a.padding), nz, ny, nx, (int32_t)none, w.sort.key[0]);
    const hipError_t e = radix_sort_pairs(w.sort, E, passes, sp_grid(radix_chunks(E), a.max_workgroups), s);
    if (e != hipSuccess) return e;
    const int32_t* key = w.sort.key[passes & 1];
    hipLaunchKernelGGL(sp_head_count_kernel, grid, blk, 0, s, key, E, (int32_t)none, w.tile);
    hipLaunchKernelGGL(scan_kernel<RADIX_SCAN_BLOCK>, dim3(1), dim3(RADIX_SCAN_BLOCK), 0, s, w.tile, sp_tiles(E), w.total);
    hipLaunchKernelGGL(sp_emit_kernel, grid, blk, 0, s, key, E, (int32_t)none, w.tile, w.total, out, a.out_capacity, a.out_indices,
                       a.out_key, a.n_out, a.status);
    return hipGetLastError();
}

hipError_t launch_sp_table(const dal3_sp_table_args* args, hipStream_t s) {
    const dal3_sp_table_args& a = *args;
    const int64_t total = (int64_t)a.kernel[0] * a.kernel[1] * a.kernel[2] * a.out_capacity;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(sp_table_kernel, dim3(sp_grid(sp_tiles(total), a.max_workgroups)), dim3(SP_BLOCK), 0, s, a.out_indices,
                       a.out_capacity, a.n_out, sp_shape(a.B, a.in_shape), sp_shape(a.B, a.out_shape),
                       sp_window(a.kernel, a.stride, a.padding), a.in_key, a.in_pos, a.in_capacity, a.n_in, a.table);
    return hipGetLastError();
}

size_t sp_conv_pack_floats(int taps, int c_in, int c_out) {
    const int64_t mt = (c_out + 31) / 32, ns4 = sp_cp(c_in) / 8;
    return (size_t)(SP_HEAD_FLOATS + mt * 32 + (int64_t)taps * ns4 * mt * 256);
}

hipError_t launch_sp_conv_pack(const FoldLayer& L, int taps, float* out, int32_t* status, hipStream_t s) {
    const int64_t total = (int64_t)sp_conv_pack_floats(taps, L.c_in, L.c_out);
    hipError_t e = launch_fill_words(out, SP_HEAD_FLOATS, 0, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sp_conv_pack_kernel, dim3(sp_grid(sp_tiles(total), 4096)), dim3(SP_BLOCK), 0, s, L, taps,
                       (L.c_out + 31) / 32, sp_cp(L.c_in) / 8, total, out, status);
    return hipGetLastError();
}

hipError_t launch_sp_conv(const dal3_sp_conv_args* args, hipStream_t s) {
    const dal3_sp_conv_args& a = *args;
    if (a.canvas) {
        const hipError_t e = launch_fill_words(
            a.canvas, (size_t)(a.canvas_B * a.c_out * a.canvas_shape[0] * a.canvas_shape[1] * a.canvas_shape[2]), 0, s);
        if (e != hipSuccess) return e;
    }
    if (a.out_capacity <= 0) return hipSuccess;
    SpConvGeom g = {};
    g.taps = a.taps, g.c_in = a.c_in, g.c_out = a.c_out, g.relu = a.relu, g.center = a.center_tap;
    g.mt_total = (a.c_out + 31) / 32;
    const int mtw = g.mt_total % 2 == 0 ? 2 : 1;
    g.n_groups = g.mt_total / mtw;
    g.ns4 = sp_cp(a.c_in) / 8;
    g.in_cap = a.in_capacity, g.out_cap = a.out_capacity;
    g.n_work = ((a.out_capacity + 31) / 32) * g.n_groups;
    g.n_out = a.n_out, g.table = a.table, g.x = a.x, g.residual = a.residual, g.y = a.y;
    g.flag = reinterpret_cast<const int32_t*>(a.packed);
    g.bias = a.packed + SP_HEAD_FLOATS;
    g.frag = reinterpret_cast<const f32x4*>(a.packed + SP_HEAD_FLOATS + g.mt_total * 32);
    g.canvas = a.canvas, g.out_idx = a.out_indices;
    g.cB = (int32_t)a.canvas_B, g.cD = a.canvas_shape[0], g.cH = a.canvas_shape[1], g.cW = a.canvas_shape[2];
    g.status = a.status;
    const dim3 grid(sp_grid((g.n_work + SP_WAVES - 1) / SP_WAVES, a.max_workgroups));
    switch (sp_cp(a.c_in)) {
        case 8: sp_launch_cp<8>(g, mtw, grid, s); break;
        case 16: sp_launch_cp<16>(g, mtw, grid, s); break;
        case 32: sp_launch_cp<32>(g, mtw, grid, s); break;
        case 64: sp_launch_cp<64>(g, mtw, grid, s); break;
        default: sp_launch_cp<128>(g, mtw, grid, s); break;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------- the backward pass
// The data gradient is launch_sp_conv itself with the roles swapped (include/dal3.h); what it needs beyond the forward's
// bookkeeping is the inverse table of a SparseConv3d. The weight gradient is the one new GEMM: per tap
// dW[k] (c_in x c_out) = X_k^T (c_in x sites) . dY (sites x c_out) on v_mfma_f32_32x32x2_f32 with the SITES as the
// contraction: input channels on the MFMA rows (A), output channels on its columns (B), lane half h supplies site 2 s + h
// of k-step s, so both operand loads are 32 consecutive floats of one row per half-wave. A wave owns one (tap, slice of
// SP_WGRAD_SLICE sites, group of CT x OT tiles): every loaded x fragment feeds OT MFMAs and every dy fragment CT. The
// slice's sites are taken 64 at a time: lane l reads table[tap][i0 + l] (one coalesced load), a chunk without a present
// neighbour is skipped by ballot and a k-step whose two sites are both absent by a scalar branch: adding the +0 products
// of absent sites never changes an accumulator, so the bits are those of the k-ordered fma chain over the present pairs.
// The partial of every (slice, tap) goes to the workspace in the parameter's layout; sp_wgrad_reduce_kernel adds the live
// slices in ascending order. The bias gradient takes the same two steps with plain column sums in a fixed order.
namespace {

constexpr int WG_SLICE = DAL3_SP_WGRAD_SLICE;
inline int64_t wg_slices(int64_t out_cap) { return (out_cap + WG_SLICE - 1) / WG_SLICE; }

__global__ __launch_bounds__(SP_BLOCK) void sp_table_transposed_kernel(const int32_t* in_idx, int64_t in_cap, const int64_t* n_in_ptr,
                                                                       SpShape in, SpShape out, SpWindow w, const int32_t* out_key,
                                                                       int64_t out_cap, const int64_t* n_out_ptr, int32_t* table) {
    const int64_t n_in = sp_live(n_in_ptr, in_cap), n_out = sp_live(n_out_ptr, out_cap);
    const int taps = w.k[0] * w.k[1] * w.k[2];
    const int64_t total = (int64_t)taps * in_cap;
    for (int64_t e = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * SP_BLOCK) {
        const int64_t j = e % in_cap;
        const int tap = (int)(e / in_cap);
        if (j >= n_in) continue;
        int32_t found = -1;
        if (sp_key_of(in_idx, j, in) >= 0) {
            const int kk[3] = {tap / (w.k[1] * w.k[2]), (tap / w.k[2]) % w.k[1], tap % w.k[2]};
            const int32_t ext[3] = {out.D, out.H, out.W};
            int32_t o[3];
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int32_t t = in_idx[4 * j + 1 + a] + w.p[a] - kk[a];      // = o * stride
                o[a] = t / w.s[a];
                if (t < 0 || o[a] * w.s[a] != t || o[a] >= ext[a]) ok = false;
            }
            if (ok) {
                const int32_t k = (int32_t)((((int64_t)in_idx[4 * j] * out.D + o[0]) * out.H + o[1]) * out.W + o[2]);
                const int64_t lo = lower_bound(out_key, 0, n_out, k);
                if (lo < n_out && out_key[lo] == k) found = (int32_t)lo;
            }
        }
        table[e] = found;
    }
}

struct SpWgradGeom {
    int taps, c_in, c_out, ci_tiles, co_tiles, ci_groups, co_groups;
    int64_t in_cap, out_cap, n_work;
    const int64_t* n_out;
    const int32_t* table;
    const float *x, *dy;
    float *part, *part_b;               // (slices, taps, c_in, c_out), (slices, c_out)
    float *dw, *db;
};

// CT x OT tiles of 32 x 32 per wave
template <int CT, int OT>
__global__ __launch_bounds__(SP_BLOCK) void sp_wgrad_kernel(const SpWgradGeom g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t n_out = sp_live(g.n_out, g.out_cap);
    const int groups = g.ci_groups * g.co_groups;
    for (int64_t work = (int64_t)blockIdx.x * SP_WAVES + wave; work < g.n_work; work += (int64_t)gridDim.x * SP_WAVES) {
        const int grp = (int)(work % groups);
        const int tap = (int)((work / groups) % g.taps);
        const int64_t slice = work / ((int64_t)groups * g.taps);
        const int64_t s0 = slice * WG_SLICE;
        if (s0 >= n_out) continue;                          // a dead slice: neither written nor summed
        const int64_t s1 = s0 + WG_SLICE < n_out ? s0 + WG_SLICE : n_out;
        const int ci0 = (grp / g.co_groups) * CT * 32 + r, co0 = (grp % g.co_groups) * OT * 32 + r;

        f32x16 acc[CT][OT];
#pragma unroll
        for (int a = 0; a < CT; ++a)
#pragma unroll
            for (int b = 0; b < OT; ++b) acc[a][b] = f32x16{};

        for (int64_t i0 = s0; i0 < s1; i0 += 64) {
            int32_t tidx = -1;
            if (i0 + lane < s1) {
                tidx = g.table[(int64_t)tap * g.out_cap + i0 + lane];
                if (tidx >= g.in_cap) tidx = -1;
            }
            if (__ballot(tidx >= 0) == 0ull) continue;
#pragma unroll 4
            for (int s = 0; s < 32; ++s) {
                const int32_t e0 = __builtin_amdgcn_readlane(tidx, 2 * s), e1 = __builtin_amdgcn_readlane(tidx, 2 * s + 1);
                if (e0 < 0 && e1 < 0) continue;             // scalar: neither site of the k-step has the tap
                const int32_t idx = h ? e1 : e0;
                const float* xr = g.x + (int64_t)(idx < 0 ? 0 : idx) * g.c_in;
                const float* dr = g.dy + (i0 + 2 * s + h) * g.c_out;
                float a[CT], b[OT];
#pragma unroll
                for (int t = 0; t < CT; ++t) a[t] = (idx >= 0 && ci0 + 32 * t < g.c_in) ? xr[ci0 + 32 * t] : 0.f;
#pragma unroll
                for (int t = 0; t < OT; ++t) b[t] = (idx >= 0 && co0 + 32 * t < g.c_out) ? dr[co0 + 32 * t] : 0.f;
#pragma unroll
                for (int ta = 0; ta < CT; ++ta)
#pragma unroll
                    for (int tb = 0; tb < OT; ++tb) acc[ta][tb] = mfma32(a[ta], b[tb], acc[ta][tb]);
            }
        }

        // register q of lane half h is input channel tile_chan(q, h) of the tile, the lane's column its output channel
        float* out = g.part + ((int64_t)slice * g.taps + tap) * g.c_in * g.c_out;
#pragma unroll
        for (int ta = 0; ta < CT; ++ta)
#pragma unroll
            for (int tb = 0; tb < OT; ++tb) {
                const int co = co0 + 32 * tb;
                if (co >= g.c_out) continue;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int ci = ci0 - r + 32 * ta + tile_chan(q, h);
                    if (ci < g.c_in) out[(int64_t)ci * g.c_out + co] = acc[ta][tb][q];
                }
            }
    }
}

// one workgroup per slice: thread t sums channel t % c_out over the rows t / c_out, t / c_out + R, ... of the slice in
// ascending order, then the R row classes are added in ascending order
__global__ __launch_bounds__(SP_BLOCK) void sp_wgrad_bias_kernel(const SpWgradGeom g, int64_t slices) {
    __shared__ float s_sum[SP_BLOCK];
    const int64_t n_out = sp_live(g.n_out, g.out_cap);
    const int R = SP_BLOCK / g.c_out, c = threadIdx.x % g.c_out, k = threadIdx.x / g.c_out;
    for (int64_t slice = blockIdx.x; slice < slices; slice += gridDim.x) {
        const int64_t s0 = slice * WG_SLICE;
        if (s0 >= n_out) break;
        const int64_t s1 = s0 + WG_SLICE < n_out ? s0 + WG_SLICE : n_out;
        float v = 0.f;
        if (k < R)
            for (int64_t i = s0 + k; i < s1; i += R) v += g.dy[i * g.c_out + c];
        s_sum[threadIdx.x] = v;
        __syncthreads();
        if (threadIdx.x < g.c_out) {
            float t = 0.f;
            for (int j = 0; j < R; ++j) t += s_sum[j * g.c_out + threadIdx.x];
            g.part_b[slice * g.c_out + threadIdx.x] = t;
        }
        __syncthreads();
    }
}

// dw = the live slices' partials in ascending slice order; db the same (the elements behind dw's)
__global__ __launch_bounds__(SP_BLOCK) void sp_wgrad_reduce_kernel(const SpWgradGeom g) {
    const int64_t n_out = sp_live(g.n_out, g.out_cap);
    const int64_t live = (n_out + WG_SLICE - 1) / WG_SLICE;
    const int64_t nw = (int64_t)g.taps * g.c_in * g.c_out, total = nw + (g.db ? g.c_out : 0);
    for (int64_t e = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * SP_BLOCK) {
        float v = 0.f;
        if (e < nw) {
            for (int64_t s = 0; s < live; ++s) v += g.part[s * nw + e];
            g.dw[e] = v;
        } else {
            for (int64_t s = 0; s < live; ++s) v += g.part_b[s * g.c_out + (e - nw)];
            g.db[e - nw] = v;
        }
    }
}

struct SpWgradWs {
    float *part, *part_b;
};
inline SpWgradWs carve_wgrad(Carver& c, int taps, int c_in, int c_out, int64_t out_cap) {
    SpWgradWs w;
    const int64_t slices = wg_slices(out_cap);
    w.part = c.take<float>((size_t)(slices * taps * c_in * c_out));
    w.part_b = c.take<float>((size_t)(slices * c_out));
    return w;
}

}  // namespace

hipError_t launch_sp_table_transposed(const dal3_sp_table_transposed_args* args, hipStream_t s) {
    const dal3_sp_table_transposed_args& a = *args;
    const int64_t total = (int64_t)a.kernel[0] * a.kernel[1] * a.kernel[2] * a.in_capacity;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(sp_table_transposed_kernel, dim3(sp_grid(sp_tiles(total), a.max_workgroups)), dim3(SP_BLOCK), 0, s,
                       a.in_indices, a.in_capacity, a.n_in, sp_shape(a.B, a.in_shape), sp_shape(a.B, a.out_shape),
                       sp_window(a.kernel, a.stride, a.padding), a.out_key, a.out_capacity, a.n_out, a.table);
    return hipGetLastError();
}

size_t sp_wgrad_workspace_bytes(int taps, int c_in, int c_out, int64_t out_capacity) {
    Carver c(nullptr, 0);
    carve_wgrad(c, taps, c_in, c_out, out_capacity);
    return c.off;
}

hipError_t launch_sp_wgrad(const dal3_sp_wgrad_args* args, hipStream_t s) {
    const dal3_sp_wgrad_args& a = *args;
    Carver c(a.workspace, a.workspace_bytes);
    const SpWgradWs w = carve_wgrad(c, a.taps, a.c_in, a.c_out, a.out_capacity);
    SpWgradGeom g = {};
    g.taps = a.taps, g.c_in = a.c_in, g.c_out = a.c_out;
    g.ci_tiles = (a.c_in + 31) / 32, g.co_tiles = (a.c_out + 31) / 32;
    const int ct = g.ci_tiles >= 2 ? 2 : 1, ot = g.co_tiles >= 4 ? 4 : g.co_tiles >= 2 ? 2 : 1;
    g.ci_groups = g.ci_tiles / ct, g.co_groups = g.co_tiles / ot;
    g.in_cap = a.in_capacity, g.out_cap = a.out_capacity;
    const int64_t slices = wg_slices(a.out_capacity);
    g.n_work = slices * a.taps * g.ci_groups * g.co_groups;
    g.n_out = a.n_out, g.table = a.table, g.x = a.x, g.dy = a.dy, g.part = w.part, g.part_b = w.part_b, g.dw = a.dw, g.db = a.db;
    if (slices > 0) {
        const dim3 grid(sp_grid((g.n_work + SP_WAVES - 1) / SP_WAVES, a.max_workgroups)), blk(SP_BLOCK);
        if (ct == 2 && ot == 4) hipLaunchKernelGGL((sp_wgrad_kernel<2, 4>), grid, blk, 0, s, g);
        else if (ct == 2 && ot == 2) hipLaunchKernelGGL((sp_wgrad_kernel<2, 2>), grid, blk, 0, s, g);
        else if (ct == 2) hipLaunchKernelGGL((sp_wgrad_kernel<2, 1>), grid, blk, 0, s, g);
        else if (ot == 4) hipLaunchKernelGGL((sp_wgrad_kernel<1, 4>), grid, blk, 0, s, g);
        else if (ot == 2) hipLaunchKernelGGL((sp_wgrad_kernel<1, 2>), grid, blk, 0, s, g);
        else hipLaunchKernelGGL((sp_wgrad_kernel<1, 1>), grid, blk, 0, s, g);
        if (a.db) hipLaunchKernelGGL(sp_wgrad_bias_kernel, dim3(sp_grid(slices, a.max_workgroups)), blk, 0, s, g, slices);
    }
    const int64_t total = (int64_t)a.taps * a.c_in * a.c_out + (a.db ? a.c_out : 0);
    hipLaunchKernelGGL(sp_wgrad_reduce_kernel, dim3(sp_grid(sp_tiles(total), a.max_workgroups)), dim3(SP_BLOCK), 0, s, g);
    return hipGetLastError();
}
