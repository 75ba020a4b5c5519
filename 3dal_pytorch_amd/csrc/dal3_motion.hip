// dal3_motion.hip — the motion-state run (dal3_group_by_key / dal3_track_features / dal3_gt_table /
// dal3_motion_classify, include/dal3.h): the regrouping of tools/trackData.py as a stable sort, trackFeature of
// tools/motionState.py:30-67, the static flag of tools/trackGT.py:60-66 and the linear decision of SVC(kernel='linear').
//
// Grouping is dal3_block.h's chunked radix sort of (key, input position) pairs. An entry that is not part of the input
// (the unused tail of a frame's slots) or whose key is outside [0, T) gets the key T and so sorts behind every group.
//
// Features are one wave per group: the float64 sums are the sequential sums NumPy forms along axis 0, taken in two
// passes (mean, then squared deviations); the integer reductions run across the lanes.
#include "dal3_block.h"
#include "dal3_kernels.h"

// no FMA contraction: the sums restate NumPy's float64 operations one by one
#pragma clang fp contract(off)

namespace {

constexpr int MO_BLOCK = 256;
constexpr int MO_WAVES = MO_BLOCK / 64;
constexpr int64_t MO_FLAG_TILE = 1024;                           // groups per compaction tile (4 per thread)

// key[2] and hist are the sort's; of the positions' ping-pong one buffer is the workspace's (pos[0] after the carve), the
// other is args.entry, which saves E words
inline RadixBufs<int32_t> carve_group(Carver& c, int64_t E) { return carve_radix<int32_t>(c, E, 1); }

struct ClassifyWs {
    int32_t* stat;                              // (tiles) each: the tiles' kept static / dynamic groups
    int32_t* dyn;
};

inline ClassifyWs carve_classify(Carver& c, int64_t T) {
    const size_t tiles = (size_t)((T + MO_FLAG_TILE - 1) / MO_FLAG_TILE);
    ClassifyWs w;
    w.stat = c.take<int32_t>(tiles);
    w.dyn = c.take<int32_t>(tiles);
    return w;
}

__device__ __forceinline__ int32_t group_key(const dal3_group_args& a, int64_t base, int64_t i) {
    const int64_t k = a.keys[i] - base;
    if (k < 0 || k >= a.T) {
        atomicOr(a.status, DAL3_MOTION_BAD_KEY);
        return (int32_t)a.T;
    }
    return (int32_t)k;
}

// the 32-bit sort key of every entry; with frames, slots [frame_offsets[f] + out_count[f], frame_offsets[f + 1]) are
// not entries
__global__ __launch_bounds__(MO_BLOCK) void group_keys_kernel(const dal3_group_args a, int32_t* key) {
    const int64_t base = (a.key_base ? *a.key_base : 0) + a.key_bias;
    if (a.frame_offsets) {
        for (int64_t f = blockIdx.x; f < a.F; f += gridDim.x) {
            const int64_t d0 = a.frame_offsets[f], d1 = a.frame_offsets[f + 1];
            int64_t n = a.out_count[f];
            if (n < 0) n = 0;
            for (int64_t i = d0 + threadIdx.x; i < d1 && i < a.E; i += MO_BLOCK) {
                if (i < 0) continue;
                key[i] = i - d0 < n ? group_key(a, base, i) : (int32_t)a.T;
            }
        }
        // slots before the first and after the last frame are no entries either
        const int64_t lo = a.F > 0 ? a.frame_offsets[0] : a.E, hi = a.F > 0 ? a.frame_offsets[a.F] : a.E;
        for (int64_t i = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x; i < a.E; i += (int64_t)gridDim.x * MO_BLOCK)
            if (i < lo || i >= hi) key[i] = (int32_t)a.T;
    } else {
        for (int64_t i = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x; i < a.E; i += (int64_t)gridDim.x * MO_BLOCK)
            key[i] = group_key(a, base, i);
    }
}

// group_start[j] = the first sorted position whose key is >= j (a binary search per group: empty groups cost the same as
// full ones); group_start[T] = the number of entries, and the key in front of it + 1 = the number of groups
__global__ __launch_bounds__(MO_BLOCK) void group_bounds_kernel(const dal3_group_args a, const int32_t* key) {
    for (int64_t j = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x; j <= a.T; j += (int64_t)gridDim.x * MO_BLOCK) {
        const int64_t lo = lower_bound(key, 0, a.E, j);
        a.group_start[j] = lo;
        if (j == a.T && a.n_groups) *a.n_groups = lo > 0 ? (int64_t)key[lo - 1] + 1 : 0;
    }
}

// ---------------------------------------------------------------------------------- features
struct Vec3 {
    double x, y, z;
};

__device__ __forceinline__ Vec3 load3(const double* c, int64_t e) { return {c[3 * e], c[3 * e + 1], c[3 * e + 2]}; }

// np.linalg.norm of a 3-vector: sqrt(x.dot(x))
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// ||c[first] - c[last]|| (motionState.py:51, trackGT.py:62)
__device__ __forceinline__ double end_distance(const double* c, int64_t first, int64_t last) {
    const Vec3 p = load3(c, first), q = load3(c, last);
    return norm3(p.x - q.x, p.y - q.y, p.z - q.z);
}

// the group's entries as a checked range: an entry outside [0, E) cannot come from dal3_group_by_key; such a group is
// treated as empty
__device__ __forceinline__ int64_t group_range(const int64_t* group_start, const int32_t* entry, int64_t g, int64_t E,
                                               int64_t& g0) {
    g0 = group_start[g];
    const int64_t g1 = group_start[g + 1];
    if (g0 < 0 || g1 > E || g1 < g0) return 0;
    for (int64_t r = g0; r < g1; ++r)
        if (entry[r] < 0 || entry[r] >= E) return 0;
    return g1 - g0;
}

// the sequential float64 sum, in entry order, of one column of a staged chunk: lanes 0..2 take x, y, z
__device__ __forceinline__ void add_chunk(const double (*s)[64], int lane, int cnt, double& acc) {
    if (lane < 3)
        for (int j = 0; j < cnt; ++j) acc += s[lane][j];
}

struct BestScore {
    float s;
    int32_t r;                                  // position inside the group
};

// np.argmax's winner of two candidates: the first NaN, else the first maximum
__device__ __forceinline__ BestScore better(BestScore a, BestScore b) {
    const bool an = a.s != a.s, bn = b.s != b.s;
    bool take_b;
    if (an || bn) take_b = bn && (!an || b.r < a.r);
    else take_b = b.s > a.s || (b.s == a.s && b.r < a.r);
    return take_b ? b : a;
}

// One wave per group. The integer reductions (sum of n_points, argmax of score) run across the lanes: they do not depend
// on the order. The float64 sums do: a chunk of 64 entries' centres is staged in LDS by all lanes, then lanes 0..2 add
// their column in entry order — mean = sum / n first, the squared deviations in a second pass over the group
// (numpy/_core/_methods.py:_var); ||.|| = sqrt(x.dot(x)). Groups from *n_groups on are empty: written as such, a
// thread each.
__global__ __launch_bounds__(MO_BLOCK) void track_features_kernel(const dal3_track_feature_args a) {
    __shared__ double s_stage[MO_WAVES][3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double(*stage)[64] = s_stage[wave];
    int64_t live = a.n_groups ? *a.n_groups : a.T;
    if (live > a.T) live = a.T;
    if (live < 0) live = 0;
    for (int64_t g = live + (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x; g < a.T; g += (int64_t)gridDim.x * MO_BLOCK) {
        a.n[g] = 0;
        a.type0[g] = 0;
        a.match_last[g] = -1;
        a.points_sum[g] = 0;
        a.best[g] = 0;
        a.keep[g] = 0;
        a.feature[2 * g] = 0.0;
        a.feature[2 * g + 1] = 0.0;
    }
    for (int64_t g = (int64_t)blockIdx.x * MO_WAVES + wave; g < live; g += (int64_t)gridDim.x * MO_WAVES) {
        int64_t g0 = a.group_start[g], n = a.group_start[g + 1] - g0;
        if (g0 < 0 || n < 0 || g0 + n > a.E) n = 0;         // not a dal3_group_by_key result: treated as empty
        // ---- integers, and the entries' range check
        int64_t points = 0;
        BestScore best = {0.f, 0x7fffffff};
        bool bad = false;
        for (int64_t r = lane; r < n; r += 64) {
            const int64_t e = a.entry[g0 + r];
            if (e < 0 || e >= a.E) {
                bad = true;
                continue;
            }
            points += a.n_points[e];
            const BestScore c = {a.score[e], (int32_t)r};
            best = best.r == 0x7fffffff ? c : better(best, c);
        }
        if (__any(bad)) n = 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            points += __shfl_xor(points, off, 64);
            const BestScore o = {__shfl_xor(best.s, off, 64), __shfl_xor(best.r, off, 64)};
            if (o.r != 0x7fffffff) best = best.r == 0x7fffffff ? o : better(best, o);
        }
        int32_t type0 = 0, match_last = -1;
        double dist = 0.0, var = 0.0;
        if (n > 0) {
            const int64_t first = a.entry[g0], last = a.entry[g0 + n - 1];
            type0 = a.type[first];
            match_last = a.match[last];
            dist = end_distance(a.center, first, last);
            // ---- the two ordered passes
            const double dn = (double)n;
            double acc = 0.0, mean[3] = {0.0, 0.0, 0.0};
            for (int pass = 0; pass < 2; ++pass) {
                acc = 0.0;
                for (int64_t c0 = 0; c0 < n; c0 += 64) {
                    const int cnt = (int)(n - c0 < 64 ? n - c0 : 64);
                    if (lane < cnt) {
                        const Vec3 p = load3(a.center, a.entry[g0 + c0 + lane]);
                        const double dx = p.x - mean[0], dy = p.y - mean[1], dz = p.z - mean[2];
                        stage[0][lane] = pass ? dx * dx : p.x;
                        stage[1][lane] = pass ? dy * dy : p.y;
                        stage[2][lane] = pass ? dz * dz : p.z;
                    }
                    __threadfence_block();      // the chunk is in LDS before lanes 0..2 read it
                    add_chunk(stage, lane, cnt, acc);
                    __threadfence_block();      // and read before the next chunk overwrites it
                }
                acc = acc / dn;
                const double q0 = __shfl(acc, 0, 64), q1 = __shfl(acc, 1, 64), q2 = __shfl(acc, 2, 64);
                if (pass == 0) {
                    mean[0] = q0;
                    mean[1] = q1;
                    mean[2] = q2;
                } else {
                    var = norm3(q0, q1, q2);
                }
            }
        }
        if (lane == 0) {
            a.n[g] = (int32_t)n;
            a.type0[g] = type0;
            a.match_last[g] = match_last;
            a.points_sum[g] = n > 0 ? points : 0;
            a.best[g] = n > 0 ? best.r : 0;
            // motionState.py:37: match == None or bbox.shape[0] < 7 or types[0] == 2 or point.shape[0] == 0
            a.keep[g] = !(match_last < 0 || n < 7 || type0 == 2 || points == 0);
            a.feature[2 * g] = dist;
            a.feature[2 * g + 1] = var;
        }
    }
}

// trackGT.py:43-46 per entry: the box moved to the global frame by its frame's veh_to_global (transform_box, :12-25)
// and the speed ||box[6:8]||
__global__ __launch_bounds__(MO_BLOCK) void gt_transform_kernel(const dal3_gt_table_args a) {
    for (int64_t e = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * MO_BLOCK) {
        const double* b = a.box + 9 * e;
        const int64_t f = a.frame[e];
        double* o = a.box_global + 7 * e;
        if (f < 0 || f >= a.F) {
            atomicOr(a.status, DAL3_MOTION_BAD_KEY);
            for (int j = 0; j < 7; ++j) o[j] = __builtin_nan("");
            a.vel[e] = __builtin_nan("");
            continue;
        }
        const double* m = a.pose + 16 * f;
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = m[4 * i] * b[0] + m[4 * i + 1] * b[1] + m[4 * i + 2] * b[2] + m[4 * i + 3];
        o[3] = b[3];
        o[4] = b[4];
        o[5] = b[5];
        o[6] = b[8] + atan2(m[4], m[0]);
        a.vel[e] = sqrt(b[6] * b[6] + b[7] * b[7]);
    }
}

// trackGT.py:60-66 per object: static = ||c[0] - c[-1]|| < 1 and max(vel) < 1 (np.max: a NaN stays)
__global__ __launch_bounds__(MO_BLOCK) void gt_table_kernel(const dal3_gt_table_args a) {
    for (int64_t g = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x; g < a.T; g += (int64_t)gridDim.x * MO_BLOCK) {
        int64_t g0;
        const int64_t n = group_range(a.group_start, a.entry, g, a.E, g0);
        double dist = 0.0, vmax = 0.0;
        if (n > 0) {
            const int64_t first = a.entry[g0], last = a.entry[g0 + n - 1];
            const double *pf = a.box_global + 7 * first, *pl = a.box_global + 7 * last;
            dist = norm3(pf[0] - pl[0], pf[1] - pl[1], pf[2] - pl[2]);
            vmax = a.vel[first];
            for (int64_t r = 1; r < n; ++r) {
                const double v = a.vel[a.entry[g0 + r]];
                if (v > vmax || (v != v && vmax == vmax)) vmax = v;
            }
        }
        a.n[g] = (int32_t)n;
        a.dist[g] = dist;
        a.max_vel[g] = vmax;
        a.is_static[g] = n > 0 && dist < 1.0 && vmax < 1.0;
    }
}

// ---------------------------------------------------------------------------------- classification
// decision = f0 * w0 + f1 * w1 + b; static = decision > 0 (scikit-learn's binary rule)
__device__ __forceinline__ bool classify_one(const dal3_motion_classify_args& a, int64_t g, double& d) {
    d = a.feature[2 * g] * a.w[0] + a.feature[2 * g + 1] * a.w[1] + a.b;
    return d > 0.0;
}

// tile = MO_FLAG_TILE consecutive groups; stat[tile] = its kept static groups, dyn[tile] = its kept dynamic ones
__global__ __launch_bounds__(MO_BLOCK) void classify_count_kernel(const dal3_motion_classify_args a, int32_t* stat, int32_t* dyn) {
    __shared__ int32_t s_n[2];
    const int64_t tiles = (a.T + MO_FLAG_TILE - 1) / MO_FLAG_TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
        __syncthreads();
        int32_t ns = 0, nd = 0;
        for (int64_t g = tile * MO_FLAG_TILE + threadIdx.x; g < a.T && g < (tile + 1) * MO_FLAG_TILE; g += MO_BLOCK) {
            double d;
            const bool st = classify_one(a, g, d);
            a.decision[g] = d;
            a.is_static[g] = st;
            ns += a.keep[g] && st;
            nd += a.keep[g] && !st;
        }
        if (ns) atomicAdd(&s_n[0], ns);
        if (nd) atomicAdd(&s_n[1], nd);
        __syncthreads();
        if (threadIdx.x < 2) (threadIdx.x == 0 ? stat : dyn)[tile] = s_n[threadIdx.x];
        __syncthreads();
    }
}

// the stable compaction: stat_start / dyn_start are the exclusive scans of the tiles' counts; inside a tile the slots go
// by group index (ballot ranks, the waves in order)
__global__ __launch_bounds__(MO_BLOCK) void classify_fill_kernel(const dal3_motion_classify_args a, const int32_t* stat_start,
                                                                 const int32_t* dyn_start) {
    __shared__ int32_t s_cnt[MO_WAVES];
    const int t = threadIdx.x;
    const int64_t tiles = (a.T + MO_FLAG_TILE - 1) / MO_FLAG_TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int32_t base[2] = {stat_start[tile], dyn_start[tile]};
        for (int64_t g0 = tile * MO_FLAG_TILE; g0 < a.T && g0 < (tile + 1) * MO_FLAG_TILE; g0 += MO_BLOCK) {
            const int64_t g = g0 + t;
            const bool kept = g < a.T && a.keep[g];
            const bool st = kept && a.is_static[g];
            for (int which = 0; which < 2; ++which) {
                const bool flag = which == 0 ? st : (kept && !st);
                int32_t total;
                const int64_t o = (int64_t)base[which] + block_rank<MO_WAVES>(flag, s_cnt, total);
                if (flag && o >= 0 && o < a.T) (which == 0 ? a.static_ids : a.dynamic_ids)[o] = (int32_t)g;
                base[which] += total;
            }
        }
    }
}

// grid-stride beyond 8 workgroups per CU
inline unsigned mo_grid(int64_t work_items, int64_t max_workgroups) { return grid_clamp(work_items, 2048, max_workgroups); }

}  // namespace

size_t group_workspace_bytes(int64_t E, int64_t T) {
    (void)T;
    Carver c(nullptr, 0);
    carve_group(c, E);
    return c.off;
}

size_t motion_classify_workspace_bytes(int64_t T) {
    Carver c(nullptr, 0);
    carve_classify(c, T);
    return c.off;
}

hipError_t launch_group_by_key(const dal3_group_args* a, hipStream_t s) {
    Carver c(a->workspace, a->workspace_bytes);
    RadixBufs<int32_t> ws = carve_group(c, a->E);
    const int64_t E = a->E;
    const int passes = radix_passes(a->T);
    const int32_t* sorted = ws.key[0];
    if (E > 0) {
        const int64_t key_items = a->frame_offsets ? (a->F > (E + MO_BLOCK - 1) / MO_BLOCK ? a->F : (E + MO_BLOCK - 1) / MO_BLOCK)
                                                   : (E + MO_BLOCK - 1) / MO_BLOCK;
        hipLaunchKernelGGL(group_keys_kernel, dim3(mo_grid(key_items, a->max_workgroups)), dim3(MO_BLOCK), 0, s, *a, ws.key[0]);
        int32_t* const own = ws.pos[0];
        ws.pos[passes & 1] = a->entry;          // where the sorted positions land
        ws.pos[~passes & 1] = own;
        const hipError_t e = radix_sort_pairs(ws, E, passes, mo_grid(radix_chunks(E), a->max_workgroups), s);
        if (e != hipSuccess) return e;
        sorted = ws.key[passes & 1];
    }
    hipLaunchKernelGGL(group_bounds_kernel, dim3(mo_grid((a->T + MO_BLOCK) / MO_BLOCK, a->max_workgroups)), dim3(MO_BLOCK), 0, s, *a,
                       sorted);
    return hipGetLastError();
}

hipError_t launch_track_features(const dal3_track_feature_args* a, hipStream_t s) {
    if (a->T == 0) return hipSuccess;
    hipLaunchKernelGGL(track_features_kernel, dim3(mo_grid((a->T + MO_WAVES - 1) / MO_WAVES, a->max_workgroups)), dim3(MO_BLOCK), 0,
                       s, *a);
    return hipGetLastError();
}

hipError_t launch_gt_table(const dal3_gt_table_args* a, hipStream_t s) {
    if (a->E > 0)
        hipLaunchKernelGGL(gt_transform_kernel, dim3(mo_grid((a->E + MO_BLOCK - 1) / MO_BLOCK, a->max_workgroups)), dim3(MO_BLOCK), 0,
                           s, *a);
    if (a->T > 0)
        hipLaunchKernelGGL(gt_table_kernel, dim3(mo_grid((a->T + MO_BLOCK - 1) / MO_BLOCK, a->max_workgroups)), dim3(MO_BLOCK), 0, s,
                           *a);
    return hipGetLastError();
}

hipError_t launch_motion_classify(const dal3_motion_classify_args* a, hipStream_t s) {
    const int64_t tiles = (a->T + MO_FLAG_TILE - 1) / MO_FLAG_TILE;
    Carver c(a->workspace, a->workspace_bytes);
    const ClassifyWs ws = carve_classify(c, a->T);
    int32_t *stat = ws.stat, *dyn = ws.dyn;
    if (tiles > 0)
        hipLaunchKernelGGL(classify_count_kernel, dim3(mo_grid(tiles, a->max_workgroups)), dim3(MO_BLOCK), 0, s, *a, stat, dyn);
    // with T == 0 the scans only write the two zero totals
    hipLaunchKernelGGL(scan_kernel<RADIX_SCAN_BLOCK>, dim3(1), dim3(RADIX_SCAN_BLOCK), 0, s, stat, tiles, a->counts);
    hipLaunchKernelGGL(scan_kernel<RADIX_SCAN_BLOCK>, dim3(1), dim3(RADIX_SCAN_BLOCK), 0, s, dyn, tiles, a->counts + 1);
    if (tiles > 0)
        hipLaunchKernelGGL(classify_fill_kernel, dim3(mo_grid(tiles, a->max_workgroups)), dim3(MO_BLOCK), 0, s, *a, stat, dyn);
    return hipGetLastError();
}
