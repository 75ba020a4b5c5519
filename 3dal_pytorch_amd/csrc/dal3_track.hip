// dal3_track.hip — the tracking run (dal3_track / dal3_track_match, include/dal3.h): CenterPoint's greedy tracker
// PubTracker.step_centertrack (tools/waymo_tracking/tracker.py) over every frame of every sequence in one launch, and
// the ground-truth match of _create_pd_detection(tracking=True) (det3d/datasets/waymo/waymo_common.py:173-189).
//
// Tracker: one workgroup per sequence (grid-stride when the grid is capped); the sequence's live tracks sit in two
// global-memory slot arrays of `capacity` entries (the old list, the new list), swapped frame by frame. A frame is
//   A  every detection row's best valid column, a wave per row (lanes over the tracks), lowest index on ties;
//   B  the greedy commit in row order by wave 0 — a row whose candidate (or first NaN) column an earlier row took is
//      re-scanned over the columns still free; the taken set is an LDS bitmap;
//   C  the new list — matched rows, new rows, kept old tracks — placed by block-wide ballot scans, and the frame's
//      output (box id, tracking id) written.
// Ids are counted per sequence from 1; dal3_track_finalize adds the exclusive scan of the per-sequence counts, so the
// ids do not depend on which workgroup ran which sequence.
#include "dal3_block.h"
#include "dal3_kernels.h"

// no FMA contraction: the distance is numpy's float32 dx*dx + dy*dy then sqrt, and the match scores pairs with the
// arithmetic of dal3_iou.hip's kernels (dal3_iou_pair.h)
#pragma clang fp contract(off)

namespace {

#include "dal3_iou_pair.h"

constexpr int TK_BLOCK = 256;
constexpr int TK_WAVES = TK_BLOCK / 64;
constexpr int32_t TK_NONE = 0x7fffffff;

struct TrackSlot {                              // 48 bytes: one entry of PubTracker.tracks
    double cx, cy;                              // 'ct' (float64, global frame)
    double tx, ty;                              // 'tracking' (float64)
    int64_t id;                                 // 'tracking_id', counted from 1 within the sequence
    int32_t label, age;                         // 'label_preds', 'age'
};

struct TrackWs {
    TrackSlot* slots;                           // (S, 2, capacity)
    int32_t* row_best;                          // (K) phase A: best valid column, -1 none
    int32_t* row_nan;                           // (K) phase A: first NaN column, TK_NONE none
    int32_t* row_col;                           // (K) phase B: the column taken, -1 none
    int64_t* seq_ids;                           // (S) new ids of each sequence
};

__host__ __device__ inline TrackWs carve_track(Carver& c, int64_t S, int64_t K, int64_t cap) {
    TrackWs w;
    w.slots = c.take<TrackSlot>((size_t)S * 2 * (size_t)cap);
    w.row_best = c.take<int32_t>((size_t)K);
    w.row_nan = c.take<int32_t>((size_t)K);
    w.row_col = c.take<int32_t>((size_t)K);
    w.seq_ids = c.take<int64_t>((size_t)S);
    return w;
}

__device__ __forceinline__ TrackWs track_ws(const dal3_track_args& a) {
    Carver c(a.workspace, a.workspace_bytes);
    return carve_track(c, a.S, a.K, a.capacity);
}

// lexicographic (value, column) minimum across the wave; NaN never enters (it is tracked apart)
__device__ __forceinline__ void wave_argmin(float& v, int32_t& j, int32_t& nan_j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int32_t oj = __shfl_xor(j, off, 64), on = __shfl_xor(nan_j, off, 64);
        if (ov < v || (ov == v && oj < j)) {
            v = ov;
            j = oj;
        }
        nan_j = min(nan_j, on);
    }
}

// the detection's position in the distance: dets = float32(ct + float32(tracking)) (tracker.py:60-62)
__device__ __forceinline__ void det_pos(const dal3_track_args& a, int64_t d, float& px, float& py) {
    px = (float)(a.ct[2 * d] + (double)(float)a.tracking[2 * d]);
    py = (float)(a.ct[2 * d + 1] + (double)(float)a.tracking[2 * d + 1]);
}

// max_diff of the detection's class (float32, tracker.py:72); a label outside 0..2 (the reference raises in
// label_to_name, test.py:172-180) matches nothing and is reported in the status word
__device__ __forceinline__ float class_max(const dal3_track_args& a, int32_t lab) {
    if (lab < 0 || lab > 2) {
        atomicOr(a.status, DAL3_TRACK_BAD_LABEL);
        return -1.f;
    }
    return a.max_dist[lab];
}

__device__ __forceinline__ bool tk_taken(const uint32_t* taken, int32_t j) { return (taken[j >> 5] >> (j & 31)) & 1u; }

// One row of the distance matrix against the tracks, columns in `taken` skipped (taken == nullptr: none), on one wave:
//   dist = sqrtf(dx*dx + dy*dy), track side = float32(ct)                               (tracker.py:66,74-78)
//   invalid = dist > max_diff[det class] (float32) or the classes differ               (tracker.py:80-81)
// Returns (wave-uniform) the lowest-index minimum over the valid columns, -1 when there is none or it is not below
// 1e16 (greedy_assignment: `dist[i][j] < 1e16`, tracker.py:11), and the first NaN column, TK_NONE when none: numpy's
// argmin returns the first NaN of the row (valid or not — NaN + 1e18 stays NaN) and NaN < 1e16 is false, so such a
// row takes nothing (tracker.py:9-12).
__device__ __forceinline__ void row_scan(const TrackSlot* old, int32_t M, float px, float py, int32_t lab, float md,
                                         const uint32_t* taken, int lane, int32_t& best, int32_t& nan_j) {
    float bv = __builtin_inff();
    int32_t bj = TK_NONE;
    nan_j = TK_NONE;
    for (int32_t j = lane; j < M; j += 64) {
        if (taken && tk_taken(taken, j)) continue;
        const float tx = (float)old[j].cx, ty = (float)old[j].cy;
        const float dx = tx - px, dy = ty - py;
        const float d = sqrtf(dx * dx + dy * dy);
        if (d != d) {
            nan_j = min(nan_j, j);
        } else if (!(d > md) && old[j].label == lab && d < bv) {
            bv = d;
            bj = j;
        }
    }
    wave_argmin(bv, bj, nan_j);
    best = (bj != TK_NONE && (double)bv < 1e16) ? bj : -1;
}

__global__ __launch_bounds__(TK_BLOCK) void track_kernel(const dal3_track_args a) {
    __shared__ uint32_t s_taken[DAL3_TRACK_MAX_CAPACITY / 32];
    __shared__ int32_t s_cnt[TK_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t cap = a.capacity;
    const TrackWs ws = track_ws(a);
    for (int64_t s = blockIdx.x; s < a.S; s += gridDim.x) {
        TrackSlot* buf[2] = {ws.slots + (2 * s) * cap, ws.slots + (2 * s + 1) * cap};
        int cur = 0;
        int32_t M = 0;                          // a sequence's first frame resets the tracks (test.py:91-93)
        int64_t n_new = 0;
        bool overflow = false;
        for (int64_t f = a.seq_offsets[s]; f < a.seq_offsets[s + 1]; ++f) {
            const int64_t d0 = a.frame_offsets[f];
            const int32_t N = (int32_t)(a.frame_offsets[f + 1] - d0);
            if (N == 0) {                       // an empty frame empties the track list (tracker.py:40-42)
                M = 0;
                if (t == 0) a.out_count[f] = 0;
                continue;
            }
            const TrackSlot* old = buf[cur];
            TrackSlot* nw = buf[cur ^ 1];
            // ---- A: each row's best valid column over all tracks
            if (M > 0) {
                for (int32_t i = wave; i < N; i += TK_WAVES) {
                    float px, py;
                    det_pos(a, d0 + i, px, py);
                    const int32_t lab = a.label[d0 + i];
                    int32_t best, nan_j;
                    row_scan(old, M, px, py, lab, class_max(a, lab), nullptr, lane, best, nan_j);
                    if (lane == 0) {
                        ws.row_best[d0 + i] = best;
                        ws.row_nan[d0 + i] = nan_j;
                    }
                }
                for (int32_t w = t; w < (M + 31) / 32; w += TK_BLOCK) s_taken[w] = 0u;
            }
            __syncthreads();
            // ---- B: greedy_assignment (tracker.py:6-15) in row order. A row's phase-A answer stands unless an earlier
            // row took its column (or its first NaN column: the next NaN, if any, then decides); such rows are re-scanned
            // over the free columns. Taking columns only removes candidates, so a row with neither a NaN nor a valid
            // column below 1e16 stays unmatched.
            if (M > 0 && wave == 0) {
                for (int32_t i = 0; i < N; ++i) {
                    const int32_t best = ws.row_best[d0 + i], nan_j = ws.row_nan[d0 + i];
                    int32_t take = -1;
                    bool rescan = false;
                    if (nan_j != TK_NONE) rescan = tk_taken(s_taken, nan_j);
                    else if (best >= 0) {
                        if (tk_taken(s_taken, best)) rescan = true;
                        else take = best;
                    }
                    if (rescan) {
                        float px, py;
                        det_pos(a, d0 + i, px, py);
                        const int32_t lab = a.label[d0 + i];
                        int32_t b2, n2;
                        row_scan(old, M, px, py, lab, class_max(a, lab), s_taken, lane, b2, n2);
                        take = n2 != TK_NONE ? -1 : b2;
                    }
                    if (lane == 0) {
                        ws.row_col[d0 + i] = take;
                        if (take >= 0) s_taken[take >> 5] |= 1u << (take & 31);
                    }
                    __threadfence_block();      // the bit is set before any lane of the wave reads the bitmap again
                }
            }
            __syncthreads();
            // ---- C: the new track list (tracker.py:96-129): matched rows in row order, then the unmatched rows scoring
            // above score_thresh (float64 compare) with new ids in row order, then the unmatched old tracks with
            // age < max_age in list order (age + 1, ct - tracking in float64; not output)
            int32_t n_match = 0, n_fresh = 0;
            for (int32_t i0 = 0; i0 < N; i0 += TK_BLOCK) {     // matched rows: output positions [0, n_match)
                const int32_t i = i0 + t;
                const int32_t col = (M > 0 && i < N) ? ws.row_col[d0 + i] : -1;
                int32_t cm;
                const int32_t rm = block_rank<TK_WAVES>(col >= 0, s_cnt, cm);
                if (col >= 0) {
                    a.box_ids[d0 + n_match + rm] = i;           // n_match + rm < N: inside the frame's rows
                    a.tracking_ids[d0 + n_match + rm] = old[col].id;
                }
                n_match += cm;
            }
            for (int32_t i0 = 0, nm = 0; i0 < N; i0 += TK_BLOCK) {     // new list slots; new rows output after the matched
                const int32_t i = i0 + t;
                const int32_t col = (M > 0 && i < N) ? ws.row_col[d0 + i] : -1;
                const bool m = col >= 0;
                const bool fresh = i < N && !m && (double)a.score[d0 + i] > a.score_thresh;
                int32_t cm, cf;
                const int32_t rm = block_rank<TK_WAVES>(m, s_cnt, cm);
                const int32_t rf = block_rank<TK_WAVES>(fresh, s_cnt, cf);
                TrackSlot e;
                int64_t slot = -1;
                if (m) {
                    slot = nm + rm;
                    e.id = old[col].id;
                } else if (fresh) {
                    slot = n_match + n_fresh + rf;
                    e.id = n_new + n_fresh + rf + 1;
                    a.box_ids[d0 + slot] = i;
                    a.tracking_ids[d0 + slot] = e.id;
                }
                if (slot >= 0 && slot < cap) {
                    e.cx = a.ct[2 * (d0 + i)];
                    e.cy = a.ct[2 * (d0 + i) + 1];
                    e.tx = a.tracking[2 * (d0 + i)];
                    e.ty = a.tracking[2 * (d0 + i) + 1];
                    e.label = a.label[d0 + i];
                    e.age = 1;
                    nw[slot] = e;
                }
                nm += cm;
                n_fresh += cf;
            }
            int32_t n_keep = 0;
            for (int32_t j0 = 0; j0 < M; j0 += TK_BLOCK) {
                const int32_t j = j0 + t;
                const bool keep = j < M && !tk_taken(s_taken, j) && old[j].age < a.max_age;
                int32_t ck;
                const int32_t rk = block_rank<TK_WAVES>(keep, s_cnt, ck);
                const int64_t slot = (int64_t)n_match + n_fresh + n_keep + rk;
                if (keep && slot < cap) {
                    TrackSlot e = old[j];
                    e.age += 1;
                    e.cx = e.cx + -e.tx;        // ct + tracking * -1 (tracker.py:124-127)
                    e.cy = e.cy + -e.ty;
                    nw[slot] = e;
                }
                n_keep += ck;
            }
            const int64_t M_new = (int64_t)n_match + n_fresh + n_keep;
            if (M_new > cap) overflow = true;   // the list is cut at the capacity: the sequence's ids are not a result
            M = (int32_t)(M_new < cap ? M_new : cap);
            n_new += n_fresh;
            if (t == 0) a.out_count[f] = n_match + n_fresh;
            cur ^= 1;
            __syncthreads();                    // the new list is complete before the next frame reads it
        }
        if (t == 0) {
            ws.seq_ids[s] = n_new;
            if (overflow) atomicOr(a.status, DAL3_TRACK_OVERFLOW);
        }
    }
}

// ids: sequence s adds id_base + sum of the earlier sequences' new ids; the total goes to id_total
__global__ __launch_bounds__(TK_BLOCK) void track_finalize_kernel(const dal3_track_args a) {
    __shared__ int64_t s_sum[TK_BLOCK];
    const int t = threadIdx.x;
    const TrackWs ws = track_ws(a);
    const int64_t base = a.id_base ? *a.id_base : 0;
    for (int64_t s = blockIdx.x; s < a.S || (s == 0 && a.S == 0); s += gridDim.x) {
        int64_t part = 0;
        for (int64_t q = t; q < s; q += TK_BLOCK) part += ws.seq_ids[q];
        s_sum[t] = part;
        __syncthreads();
        for (int h = TK_BLOCK / 2; h > 0; h >>= 1) {
            if (t < h) s_sum[t] += s_sum[t + h];
            __syncthreads();
        }
        const int64_t off = base + s_sum[0];
        __syncthreads();
        if (s < a.S) {
            for (int64_t f = a.seq_offsets[s]; f < a.seq_offsets[s + 1]; ++f) {
                const int64_t d0 = a.frame_offsets[f];
                for (int32_t r = t; r < a.out_count[f]; r += TK_BLOCK) a.tracking_ids[d0 + r] += off;
            }
        }
        if (t == 0 && a.id_total && s + 1 >= a.S) *a.id_total = off + (a.S > 0 ? ws.seq_ids[s] : 0);
    }
}

// ---------------------------------------------------------------------------------- ground-truth match
struct MatchWs {
    unsigned long long* first;                  // (K) per id - id_base - 1: the first output position with a candidate
    int32_t* cand_frame;                        // (K) per output position
    int32_t* cand_obj;                          // (K) the frame's annotation index with IoU > thr, -1 none
};

__host__ __device__ inline MatchWs carve_match(Carver& c, int64_t K) {
    MatchWs w;
    w.first = c.take<unsigned long long>((size_t)K);
    w.cand_frame = c.take<int32_t>((size_t)K);
    w.cand_obj = c.take<int32_t>((size_t)K);
    return w;
}

__device__ __forceinline__ MatchWs match_ws(const dal3_track_match_args& a) {
    Carver c(a.workspace, a.workspace_bytes);
    return carve_match(c, a.K);
}

__global__ __launch_bounds__(TK_BLOCK) void match_init_kernel(const dal3_track_match_args a) {
    const MatchWs ws = match_ws(a);
    for (int64_t k = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x; k < a.K; k += (int64_t)gridDim.x * TK_BLOCK)
        ws.first[k] = ~0ull;
}

// one workgroup per frame: every output detection against the frame's annotation boxes, iou_3d of (det, gt) as
// boxes_iou3d_gpu(det3d_t, bboxs_t); np.argmax's first maximum, a NaN anywhere in the row wins the argmax and fails
// `> thr` (waymo_common.py:181-188)
__global__ __launch_bounds__(TK_BLOCK) void match_candidates_kernel(const dal3_track_match_args a) {
    const MatchWs ws = match_ws(a);
    const int64_t base = a.id_base ? *a.id_base : 0;
    for (int64_t f = blockIdx.x; f < a.F; f += gridDim.x) {
        const int64_t d0 = a.frame_offsets[f], g0 = a.gt_offsets[f], G = a.gt_offsets[f + 1] - g0;
        for (int32_t r = threadIdx.x; r < a.out_count[f]; r += TK_BLOCK) {
            const int64_t k = d0 + r;
            const IouBox<float> det = iou_box<float>(a.boxes + 7 * (d0 + a.box_ids[k]));
            float bv = 0.f;
            int32_t bj = -1;
            bool nan = false;
            for (int64_t g = 0; g < G; ++g) {
                float vb, v3;
                box_iou_pair(det, iou_box<float>(a.gt_boxes + 7 * (g0 + g)), vb, v3);
                if (v3 != v3) {
                    nan = true;
                    break;
                }
                if (bj < 0 || v3 > bv) {
                    bv = v3;
                    bj = (int32_t)g;
                }
            }
            const int32_t cand = (!nan && bj >= 0 && bv > a.thr) ? bj : -1;
            ws.cand_frame[k] = (int32_t)f;
            ws.cand_obj[k] = cand;
            if (cand >= 0) {
                const int64_t idx = a.tracking_ids[k] - base - 1;
                if (idx >= 0 && idx < a.K) atomicMin(&ws.first[idx], (unsigned long long)k);
                else atomicOr(a.status, DAL3_TRACK_BAD_ID);
            }
        }
    }
}

// an id's match from its first candidate on (`matching[o.object.id]`, waymo_common.py:176-177); None before it
__global__ __launch_bounds__(TK_BLOCK) void match_fill_kernel(const dal3_track_match_args a) {
    const MatchWs ws = match_ws(a);
    const int64_t base = a.id_base ? *a.id_base : 0;
    for (int64_t f = blockIdx.x; f < a.F; f += gridDim.x) {
        const int64_t d0 = a.frame_offsets[f];
        for (int32_t r = threadIdx.x; r < a.out_count[f]; r += TK_BLOCK) {
            const int64_t k = d0 + r;
            const int64_t idx = a.tracking_ids[k] - base - 1;
            const unsigned long long fk = (idx >= 0 && idx < a.K) ? ws.first[idx] : ~0ull;
            const bool hit = fk <= (unsigned long long)k;
            a.match_frame[k] = hit ? ws.cand_frame[fk] : -1;
            a.match_obj[k] = hit ? ws.cand_obj[fk] : -1;
        }
    }
}

}  // namespace

size_t track_workspace_bytes(int64_t S, int64_t K, int64_t capacity) {
    Carver c(nullptr, 0);
    carve_track(c, S, K, capacity);
    return c.off;
}

size_t track_match_workspace_bytes(int64_t K) {
    Carver c(nullptr, 0);
    carve_match(c, K);
    return c.off;
}

hipError_t launch_track(const dal3_track_args* a, hipStream_t s) {
    const dim3 grid(grid_clamp(a->S, GRID_MAX, a->max_workgroups));
    if (a->S > 0) hipLaunchKernelGGL(track_kernel, grid, dim3(TK_BLOCK), 0, s, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_finalize_kernel, grid, dim3(TK_BLOCK), 0, s, *a);
    return hipGetLastError();
}

hipError_t launch_track_match(const dal3_track_match_args* a, hipStream_t s) {
    if (a->K == 0 || a->F == 0) return hipSuccess;
    hipLaunchKernelGGL(match_init_kernel, dim3(grid_clamp((a->K + TK_BLOCK - 1) / TK_BLOCK, 65535, 0)), dim3(TK_BLOCK), 0, s, *a);
    const unsigned gf = grid_clamp(a->F, 65535, 0);
    hipLaunchKernelGGL(match_candidates_kernel, dim3(gf), dim3(TK_BLOCK), 0, s, *a);
    hipLaunchKernelGGL(match_fill_kernel, dim3(gf), dim3(TK_BLOCK), 0, s, *a);
    return hipGetLastError();
}
