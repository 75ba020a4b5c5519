// dal3_pillars.hip — the PointPillars reader (dal3_voxelize / dal3_pillar_pack / dal3_pillar_features /
// dal3_pillar_scatter / dal3_voxel_mean, include/dal3.h): points_to_voxel of det3d/ops/point_cloud/point_cloud_ops.py,
// PillarFeatureNet and PointPillarsScatter of det3d/models/readers/pillar_encoder.py, VoxelFeatureExtractorV3 of
// voxel_encoder.py.
//
// Voxelisation restates the reference's sequential loop as an ordered compaction. Every point gets the 32-bit key
// sample * cells + cell (a point outside the range, with a NaN coordinate or outside every sample: B * cells, behind
// every real key). dal3_block.h's chunked radix sort of (key, point index) pairs, stable, leaves the points of a cell
// together and by ascending index. Then
//   heads   the first entry of a run is the cell's first point: flagged at its ORIGINAL position; every entry learns
//           where its run starts (a binary search over the sorted keys);
//   ranks   an exclusive scan of the flags in point order (per 256-point tile: count, scan of the counts, ballot ranks)
//           minus the scan at the sample's first point is the cell's rank by first appearance: the voxel index;
//   fill    an entry's place in its run is its row; rows >= max_points and cells of rank >= max_voxels are dropped.
// Every count is an integer and every output slot a function of the input alone: no atomic decides a position.
//
// The feature kernel is one wave per pillar with channels on the MFMA rows and the pillar's rows on the columns
// (dal3_device.h): layer 1's accumulators are layer 2's B operand, and so are the lanes' copies of layer 1's maximum,
// which makes the per-pillar term W2b' max1 + b2' sixteen more k-steps into the accumulators layer 2 starts from.
#include "dal3_block.h"
#include "dal3_kernels.h"

// the decoration restates torch's float32 operations one by one: no FMA contraction
#pragma clang fp contract(off)

namespace {

constexpr int PL_BLOCK = 256;
constexpr int PL_WAVES = PL_BLOCK / 64;
__host__ __device__ inline int64_t pl_tiles(int64_t N) { return (N + PL_BLOCK - 1) / PL_BLOCK; }

struct VoxWs {
    RadixBufs<int32_t> sort;                    // the (key, point index) pairs; both position buffers are the workspace's
    int32_t* start;                             // (N) where the run of sorted entry r starts
    int32_t* rank;                              // (N) by point: the head's rank among all heads, -1 for the others
    int32_t* tile;                              // (tiles) heads per 256-point tile, then their exclusive scan
    int64_t* total;                             // (1) all heads
    int64_t* base;                              // (B + 1) heads in front of each sample's first point
};

inline VoxWs carve_vox(Carver& c, int64_t B, int64_t N) {
    VoxWs w;
    w.sort = carve_radix<int32_t>(c, N, 2);
    w.start = c.take<int32_t>((size_t)N);
    w.rank = c.take<int32_t>((size_t)N);
    w.tile = c.take<int32_t>((size_t)pl_tiles(N));
    w.total = c.take<int64_t>(1);
    w.base = c.take<int64_t>((size_t)B + 1);
    return w;
}

__host__ __device__ inline int64_t vox_cells(const dal3_voxelize_args& a) {
    return (int64_t)a.grid[0] * a.grid[1] * a.grid[2];
}

// the sample of point i by the device offsets: the last b with offsets[b] <= i, -1 when i is in no sample
__device__ __forceinline__ int64_t sample_of(const int64_t* off, int64_t B, int64_t i) {
    const int64_t lo = upper_bound(off, 0, B + 1, i);       // first b with off[b] > i
    return lo >= 1 && lo <= B ? lo - 1 : -1;
}

__global__ __launch_bounds__(PL_BLOCK) void vox_keys_kernel(const dal3_voxelize_args a, int32_t* key) {
    const int64_t cells = vox_cells(a);
    const int32_t none = (int32_t)(a.B * cells);
    for (int64_t i = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; i < a.N; i += (int64_t)gridDim.x * PL_BLOCK) {
        const int64_t b = sample_of(a.point_offsets, a.B, i);
        const float* p = a.points + i * a.point_stride;
        bool ok = b >= 0;
        int32_t c[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float f = floorf(__fdiv_rn(p[j] - a.pc_range[j], a.voxel_size[j]));
            if (!(f >= 0.f) || !(f < (float)a.grid[j])) ok = false;     // a NaN fails both
            else c[j] = (int32_t)f;
        }
        key[i] = ok ? (int32_t)(b * cells + ((int64_t)c[2] * a.grid[1] + c[1]) * a.grid[0] + c[0]) : none;
    }
}

// per sorted entry: where its run starts, and the head's flag at the head's own point (rank 0 / -1 until vox_rank_kernel)
__global__ __launch_bounds__(PL_BLOCK) void vox_heads_kernel(const int32_t* key, const int32_t* pos, int64_t N, int32_t none,
                                                             int32_t* start, int32_t* rank) {
    for (int64_t r = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; r < N; r += (int64_t)gridDim.x * PL_BLOCK) {
        const int32_t k = key[r];
        const int32_t p = pos[r];
        if (p < 0 || p >= N) continue;          // cannot come from the sort
        if (k >= none) {
            rank[p] = -1;
            start[r] = (int32_t)r;
            continue;
        }
        const int64_t lo = lower_bound(key, 0, r, k);      // the first entry with this key
        start[r] = (int32_t)lo;
        rank[p] = lo == r ? 0 : -1;
    }
}

__global__ __launch_bounds__(PL_BLOCK) void vox_tile_count_kernel(const int32_t* rank, int64_t N, int32_t* tile) {
    __shared__ int32_t s_cnt[PL_WAVES];
    const int64_t tiles = pl_tiles(N);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i = t * PL_BLOCK + threadIdx.x;
        int32_t total;
        block_rank<PL_WAVES>(i < N && rank[i] >= 0, s_cnt, total);
        if (threadIdx.x == 0) tile[t] = total;
    }
}

// tile: scanned. A head's rank among all heads, in point order
__global__ __launch_bounds__(PL_BLOCK) void vox_rank_kernel(int32_t* rank, int64_t N, const int32_t* tile) {
    __shared__ int32_t s_cnt[PL_WAVES];
    const int64_t tiles = pl_tiles(N);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i = t * PL_BLOCK + threadIdx.x;
        const bool head = i < N && rank[i] >= 0;
        int32_t total;
        const int32_t r = block_rank<PL_WAVES>(head, s_cnt, total);
        if (head) rank[i] = tile[t] + r;
    }
}

// ONE workgroup: the heads in front of every sample's first point, then where each sample's voxels begin
__global__ __launch_bounds__(PL_BLOCK) void vox_offsets_kernel(const dal3_voxelize_args a, const VoxWs w) {
    for (int64_t b = threadIdx.x; b <= a.B; b += PL_BLOCK) {
        int64_t o = a.point_offsets[b];
        o = o < 0 ? 0 : o > a.N ? a.N : o;
        int64_t n = *w.total;
        if (o < a.N) {
            const int64_t t = o / PL_BLOCK;
            n = w.tile[t];
            for (int64_t i = t * PL_BLOCK; i < o; ++i) n += w.rank[i] >= 0;
        }
        w.base[b] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t at = 0;
        a.voxel_offsets[0] = 0;
        for (int64_t b = 0; b < a.B; ++b) {
            int64_t n = w.base[b + 1] - w.base[b];
            n = n < 0 ? 0 : n > a.max_voxels ? a.max_voxels : n;
            at += n;
            a.voxel_offsets[b + 1] = at;
        }
    }
}

__global__ __launch_bounds__(PL_BLOCK) void vox_fill_kernel(const dal3_voxelize_args a, const VoxWs w, const int32_t* key,
                                                            const int32_t* pos) {
    const int64_t cells = vox_cells(a);
    const int32_t none = (int32_t)(a.B * cells);
    for (int64_t r = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; r < a.N; r += (int64_t)gridDim.x * PL_BLOCK) {
        const int32_t k = key[r];
        if (k < 0 || k >= none) continue;
        const int64_t s = w.start[r];
        const int64_t row = r - s;
        if (s < 0 || row < 0 || row >= a.max_points) continue;
        const int64_t head = pos[s], me = pos[r];
        if (head < 0 || head >= a.N || me < 0 || me >= a.N) continue;
        const int64_t b = k / cells;
        const int64_t v = (int64_t)w.rank[head] - w.base[b];
        if (v < 0 || v >= a.max_voxels) continue;
        const int64_t slot = a.voxel_offsets[b] + v;
        if (slot < 0 || slot >= a.capacity) {
            atomicOr(a.status, DAL3_PILLAR_OVERFLOW);
            continue;
        }
        const float* p = a.points + me * a.point_stride;
        float* o = a.voxels + (slot * a.max_points + row) * a.C;
        for (int c = 0; c < a.C; ++c) o[c] = p[c];
        if (row == 0) {
            const int64_t n = upper_bound(key, r, a.N, k) - s;      // the first entry behind the run
            a.num_points[slot] = (int32_t)(n < a.max_points ? n : a.max_points);
            const int64_t cell = k - b * cells;
            const int32_t x = (int32_t)(cell % a.grid[0]), y = (int32_t)((cell / a.grid[0]) % a.grid[1]);
            const int32_t z = (int32_t)(cell / ((int64_t)a.grid[0] * a.grid[1]));
            int32_t* co = a.coordinates + 4 * slot;
            co[0] = (int32_t)b;
            co[1] = a.reverse_index ? z : x;
            co[2] = y;
            co[3] = a.reverse_index ? x : z;
        }
    }
}

inline unsigned pl_grid(int64_t want, int64_t max_workgroups) { return grid_clamp(want, 65535 * 16, max_workgroups); }

// ---------------------------------------------------------------------------------- pillar features
// the packed blob, in floats (include/dal3.h DAL3_PILLAR_PACK_FLOATS)
constexpr int PF_KS = 7;                        // k-steps of layer 1: C + 5 <= 13 inputs, two a step
constexpr int PF_A1 = 0;                        // [2 out-tiles][PF_KS][64 lanes]: W1'[32 mt + (l & 31)][2 s + (l >> 5)]
constexpr int PF_B1 = PF_A1 + 2 * PF_KS * 64;   // 64
constexpr int PF_A2A = PF_B1 + 64;              // [2][16][64]: W2'[32 mt + (l & 31)][tile_chan(s, l >> 5)]
constexpr int PF_A2B = PF_A2A + 2 * 16 * 64;    // [2][16][64]: W2'[32 mt + (l & 31)][32 + tile_chan(s, l >> 5)]
constexpr int PF_B2 = PF_A2B + 2 * 16 * 64;     // 64
constexpr int PF_FLOATS = PF_B2 + 64;
static_assert(PF_FLOATS == DAL3_PILLAR_PACK_FLOATS, "the header's blob size");

struct PackLayer {
    const float *w, *g, *beta, *mean, *var;
    int c_in, c_out;
};

// Not dal3_fold.h's fold: the bias here is beta - mean * scale without pinned roundings (the compiler may contract it
// into an fma), so moving this pack onto the shared fold could change its bits. It keeps its own two functions.
__device__ __forceinline__ float folded_weight(const PackLayer& L, int row, int col, double eps) {
    if (row >= L.c_out || col >= L.c_in) return 0.f;
    const double scale = (double)L.g[row] / sqrt((double)L.var[row] + eps);
    return (float)((double)L.w[(int64_t)row * L.c_in + col] * scale);
}

__device__ __forceinline__ float folded_bias(const PackLayer& L, int row, double eps) {
    if (row >= L.c_out) return 0.f;
    const double scale = (double)L.g[row] / sqrt((double)L.var[row] + eps);
    return (float)((double)L.beta[row] - (double)L.mean[row] * scale);
}

__global__ __launch_bounds__(PL_BLOCK) void pillar_pack_kernel(const PackLayer l1, const PackLayer l2, int n_layers, double eps,
                                                               float* out) {
    for (int i = blockIdx.x * PL_BLOCK + threadIdx.x; i < PF_FLOATS; i += gridDim.x * PL_BLOCK) {
        float v = 0.f;
        if (i < PF_B1) {
            const int l = i & 63, s = (i >> 6) % PF_KS, mt = (i >> 6) / PF_KS;
            v = folded_weight(l1, 32 * mt + (l & 31), 2 * s + (l >> 5), eps);
        } else if (i < PF_A2A) {
            v = folded_bias(l1, i - PF_B1, eps);
        } else if (i < PF_B2) {
            if (n_layers == 2) {
                const int j = i - PF_A2A, l = j & 63, s = (j >> 6) & 15, mt = (j >> 10) & 1, half = j >> 11;
                v = folded_weight(l2, 32 * mt + (l & 31), 32 * half + tile_chan(s, l >> 5), eps);
            }
        } else if (n_layers == 2) {
            v = folded_bias(l2, i - PF_B2, eps);
        }
        out[i] = v;
    }
}

__device__ __forceinline__ f32x16 max16(f32x16 a, f32x16 b) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = fmaxf(a[r], b[r]);
    return a;
}

// every lane of a half gets the maximum over the half's 32 columns
__device__ __forceinline__ f32x16 max_over_columns(f32x16 a) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = fmaxf(a[r], __shfl_xor(a[r], off, 64));
    }
    return a;
}

// channel 32 mt + tile_chan(r, h) of the pillar, from lanes 0..15 of each half (lane n holds register n)
__device__ __forceinline__ void store_channels(const dal3_pillar_feature_args& a, const f32x16& m, int mt, int lane, int64_t p,
                                               const int32_t* co) {
    const int n = lane & 31, h = lane >> 5;
    float v = m[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) v = n == r ? m[r] : v;
    if (n >= 16) return;
    const int ch = 32 * mt + tile_chan(n, h);
    if (a.canvas) {
        const int64_t b = co[0], y = co[2], x = co[3];
        if (b < 0 || b >= a.canvas_B || y < 0 || y >= a.ny || x < 0 || x >= a.nx) return;
        a.canvas[((b * a.c_out + ch) * a.ny + y) * a.nx + x] = v;
    } else {
        a.features[p * a.c_out + ch] = v;
    }
}

// MT1: output tiles of layer 1 (1: 32 channels and a second layer, 2: the one-layer net's 64); NT: column tiles
template <int MT1, int NT>
__global__ __launch_bounds__(PL_BLOCK) void pillar_feature_kernel(const dal3_pillar_feature_args a) {
    constexpr bool L2 = MT1 == 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
    int64_t P = a.P;
    if (a.n_pillars) {
        const int64_t live = *a.n_pillars;
        P = live < 0 ? 0 : live < P ? live : P;
    }
    // the A operands stay in registers over the wave's pillars
    float a1[MT1][PF_KS], a2a[L2 ? 2 : 1][16], a2b[L2 ? 2 : 1][16];
#pragma unroll
    for (int mt = 0; mt < MT1; ++mt) {
#pragma unroll
        for (int s = 0; s < PF_KS; ++s) a1[mt][s] = a.packed[PF_A1 + (mt * PF_KS + s) * 64 + lane];
    }
    if constexpr (L2) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                a2a[mt][s] = a.packed[PF_A2A + (mt * 16 + s) * 64 + lane];
                a2b[mt][s] = a.packed[PF_A2B + (mt * 16 + s) * 64 + lane];
            }
        }
    }
    for (int64_t p = (int64_t)blockIdx.x * PL_WAVES + wave; p < P; p += (int64_t)gridDim.x * PL_WAVES) {
        const float* vox = a.voxels + p * a.max_points * a.C;
        const int32_t* co = a.coordinates + 4 * p;
        const int32_t np = a.num_points[p];
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int r = 0; r < a.max_points; ++r) {
            sx += vox[r * a.C];
            sy += vox[r * a.C + 1];
            sz += vox[r * a.C + 2];
        }
        const float cnt = (float)np;
        const float mx = __fdiv_rn(sx, cnt), my = __fdiv_rn(sy, cnt), mz = __fdiv_rn(sz, cnt);
        const float cx = (float)co[3] * a.vx + a.x_offset, cy = (float)co[2] * a.vy + a.y_offset;
        // ---- layer 1
        f32x16 x1[NT][MT1];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int r = 32 * j + n;
            r = r < a.max_points ? r : a.max_points - 1;        // columns beyond the pillar repeat its last row
            const float* row = vox + r * a.C;
            float f[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) f[c] = c < a.C ? row[c] : 0.f;
            const float dec[5] = {f[0] - mx, f[1] - my, f[2] - mz, f[0] - cx, f[1] - cy};
            const float mask = r < np ? 1.f : 0.f;
            // this lane's B operand of k-step s: input 2 s + h of its row
            float in[PF_KS];
#pragma unroll
            for (int s = 0; s < PF_KS; ++s) {
                const int k = 2 * s + h;
                float v = 0.f;
#pragma unroll
                for (int d = 0; d < 5; ++d) v = k - a.C == d ? dec[d] : v;
#pragma unroll
                for (int c = 0; c < 8; ++c) v = k == c && c < a.C ? f[c] : v;
                in[s] = v * mask;
            }
#pragma unroll
            for (int mt = 0; mt < MT1; ++mt) {
                f32x16 acc = tile_from_channels(a.packed + PF_B1 + 32 * mt, h);
#pragma unroll
                for (int s = 0; s < PF_KS; ++s) acc = mfma32(a1[mt][s], in[s], acc);
                x1[j][mt] = relu16(acc);
            }
        }
        f32x16 max1[MT1];
#pragma unroll
        for (int mt = 0; mt < MT1; ++mt) {
            max1[mt] = x1[0][mt];
#pragma unroll
            for (int j = 1; j < NT; ++j) max1[mt] = max16(max1[mt], x1[j][mt]);
            max1[mt] = max_over_columns(max1[mt]);
        }
        if constexpr (!L2) {
#pragma unroll
            for (int mt = 0; mt < MT1; ++mt) store_channels(a, max1[mt], mt, lane, p, co);
        } else {
        // ---- layer 2: the per-pillar term first, then the rows
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x16 term = tile_from_channels(a.packed + PF_B2 + 32 * mt, h);
#pragma unroll
            for (int s = 0; s < 16; ++s) term = mfma32(a2b[mt][s], max1[0][s], term);
            f32x16 best;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                f32x16 acc = term;
#pragma unroll
                for (int s = 0; s < 16; ++s) acc = mfma32(a2a[mt][s], x1[j][0][s], acc);
                best = j == 0 ? acc : max16(best, acc);
            }
            store_channels(a, max_over_columns(relu16(best)), mt, lane, p, co);
        }
        }
    }
}

__global__ __launch_bounds__(PL_BLOCK) void pillar_scatter_kernel(const float* features, const int32_t* coordinates, int64_t P,
                                                                  const int64_t* n_pillars, int c_out, float* canvas,
                                                                  int64_t canvas_B, int64_t ny, int64_t nx) {
    if (n_pillars) {
        const int64_t live = *n_pillars;
        P = live < 0 ? 0 : live < P ? live : P;
    }
    for (int64_t i = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; i < P * c_out; i += (int64_t)gridDim.x * PL_BLOCK) {
        const int64_t p = i / c_out, ch = i % c_out;
        const int32_t* co = coordinates + 4 * p;
        const int64_t b = co[0], y = co[2], x = co[3];
        if (b < 0 || b >= canvas_B || y < 0 || y >= ny || x < 0 || x >= nx) continue;
        canvas[((b * c_out + ch) * ny + y) * nx + x] = features[i];
    }
}

__global__ __launch_bounds__(PL_BLOCK) void voxel_mean_kernel(const float* voxels, const int32_t* num_points, int64_t P,
                                                              const int64_t* n_pillars, int max_points, int C, float* out) {
    if (n_pillars) {
        const int64_t live = *n_pillars;
        P = live < 0 ? 0 : live < P ? live : P;
    }
    for (int64_t i = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; i < P * C; i += (int64_t)gridDim.x * PL_BLOCK) {
        const int64_t p = i / C, c = i % C;
        const float* v = voxels + p * max_points * C + c;
        float s = 0.f;
        for (int r = 0; r < max_points; ++r) s += v[(int64_t)r * C];
        out[i] = __fdiv_rn(s, (float)num_points[p]);
    }
}

}  // namespace

size_t voxelize_workspace_bytes(int64_t B, int64_t N) {
    Carver c(nullptr, 0);
    carve_vox(c, B, N);
    return c.off;
}

hipError_t launch_voxelize(const dal3_voxelize_args* args, hipStream_t s) {
    const dal3_voxelize_args& a = *args;
    hipError_t e;
    // rows nobody fills are zero: the padding of a voxel, and everything behind the last voxel
    if ((e = launch_fill_words(a.voxels, (size_t)a.capacity * a.max_points * a.C, 0, s)) != hipSuccess) return e;
    if ((e = launch_fill_words(a.coordinates, (size_t)a.capacity * 4, 0, s)) != hipSuccess) return e;
    if ((e = launch_fill_words(a.num_points, (size_t)a.capacity, 0, s)) != hipSuccess) return e;
    if ((e = launch_fill_words(a.voxel_offsets, ((size_t)a.B + 1) * 2, 0, s)) != hipSuccess) return e;
    if (a.B <= 0 || a.N <= 0) return hipSuccess;
    Carver c(a.workspace, a.workspace_bytes);
    const VoxWs w = carve_vox(c, a.B, a.N);
    const int64_t cells = vox_cells(a), none = a.B * cells;
    const int passes = radix_passes(none);
    const dim3 blk(PL_BLOCK);
    const dim3 g_pts(pl_grid(pl_tiles(a.N), a.max_workgroups));
    hipLaunchKernelGGL(vox_keys_kernel, g_pts, blk, 0, s, a, w.sort.key[0]);
    if ((e = radix_sort_pairs(w.sort, a.N, passes, pl_grid(radix_chunks(a.N), a.max_workgroups), s)) != hipSuccess) return e;
    const int32_t *key = w.sort.key[passes & 1], *pos = w.sort.pos[passes & 1];
    hipLaunchKernelGGL(vox_heads_kernel, g_pts, blk, 0, s, key, pos, a.N, (int32_t)none, w.start, w.rank);
    hipLaunchKernelGGL(vox_tile_count_kernel, g_pts, blk, 0, s, w.rank, a.N, w.tile);
    hipLaunchKernelGGL(scan_kernel<RADIX_SCAN_BLOCK>, dim3(1), dim3(RADIX_SCAN_BLOCK), 0, s, w.tile, pl_tiles(a.N), w.total);
    hipLaunchKernelGGL(vox_rank_kernel, g_pts, blk, 0, s, w.rank, a.N, w.tile);
    hipLaunchKernelGGL(vox_offsets_kernel, dim3(1), blk, 0, s, a, w);
    hipLaunchKernelGGL(vox_fill_kernel, g_pts, blk, 0, s, a, w, key, pos);
    return hipGetLastError();
}

hipError_t launch_pillar_pack(const dal3_layer* layers, int n_layers, double eps, float* out, hipStream_t s) {
    PackLayer l[2] = {};
    for (int i = 0; i < n_layers; ++i)
        l[i] = {layers[i].weight, layers[i].bn_weight, layers[i].bn_bias, layers[i].bn_mean, layers[i].bn_var, layers[i].c_in,
                layers[i].c_out};
    hipLaunchKernelGGL(pillar_pack_kernel, dim3((PF_FLOATS + PL_BLOCK - 1) / PL_BLOCK), dim3(PL_BLOCK), 0, s, l[0], l[1], n_layers,
                       eps, out);
    return hipGetLastError();
}

hipError_t launch_pillar_features(const dal3_pillar_feature_args* args, hipStream_t s) {
    const dal3_pillar_feature_args& a = *args;
    if (a.canvas) {
        const hipError_t e = launch_fill_words(a.canvas, (size_t)(a.canvas_B * a.c_out * a.ny * a.nx), 0, s);
        if (e != hipSuccess) return e;
    }
    if (a.P <= 0) return hipSuccess;
    const dim3 g(pl_grid((a.P + PL_WAVES - 1) / PL_WAVES, a.max_workgroups > 0 ? a.max_workgroups : 4096)), blk(PL_BLOCK);
    const bool two = a.max_points > 32;
    if (a.n_layers == 2) {
        if (two) hipLaunchKernelGGL((pillar_feature_kernel<1, 2>), g, blk, 0, s, a);
        else hipLaunchKernelGGL((pillar_feature_kernel<1, 1>), g, blk, 0, s, a);
    } else {
        if (two) hipLaunchKernelGGL((pillar_feature_kernel<2, 2>), g, blk, 0, s, a);
        else hipLaunchKernelGGL((pillar_feature_kernel<2, 1>), g, blk, 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_pillar_scatter(const float* features, const int32_t* coordinates, int64_t P, const int64_t* n_pillars, int c_out,
                                 float* canvas, int64_t canvas_B, int64_t ny, int64_t nx, hipStream_t s) {
    const hipError_t e = launch_fill_words(canvas, (size_t)(canvas_B * c_out * ny * nx), 0, s);
    if (e != hipSuccess) return e;
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(pillar_scatter_kernel, dim3(pl_grid((P * c_out + PL_BLOCK - 1) / PL_BLOCK, 0)), dim3(PL_BLOCK), 0, s,
                       features, coordinates, P, n_pillars, c_out, canvas, canvas_B, ny, nx);
    return hipGetLastError();
}

hipError_t launch_voxel_mean(const float* voxels, const int32_t* num_points, int64_t P, const int64_t* n_pillars, int max_points,
                             int C, float* out, hipStream_t s) {
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(voxel_mean_kernel, dim3(pl_grid((P * C + PL_BLOCK - 1) / PL_BLOCK, 0)), dim3(PL_BLOCK), 0, s, voxels,
                       num_points, P, n_pillars, max_points, C, out);
    return hipGetLastError();
}
