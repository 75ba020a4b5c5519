// dal3_roi.hip — CenterPoint's second stage (dal3_bev_gather, dal3_box_points, dal3_roi_pack, dal3_roi_head,
// dal3_roi_post of include/dal3.h, whose comment is the definition): the fused route from the first stage's kept rows to
// refined boxes in three launches on the caller's stream.
//
//   roi_prepare_kernel   one thread per (sample, slot): walks the sample's tasks over keep_count to find the slot's kept
//                        row (T <= 16 segments: a walk, not a scan), writes the roi with the rotation at column 6, its
//                        score and label, the num_point points and their sample (-1: a slot past the count);
//   bev_gather_kernel    one wave per point, the lanes over the channels; the four weights are wave-uniform;
//   roi_mlp_kernel       one workgroup (8 waves) per 32 slots of one sample. In the orientation of dal3_device.h: output
//                        channels on the MFMA rows, the 32 RoIs on its columns (= lanes), two inputs per k-step. The
//                        first layer (K = num_point * C, up to 8 out tiles: one per wave) stages the feature rows 64
//                        inputs at a time, transposed into LDS (a row of 33 floats per input: the transposing store
//                        meets no bank twice), and sums each chunk from zero before adding it to the total, as
//                        dal3_conv2d does. Every later layer reads its input tile [channel][32] from LDS and writes
//                        its output tile there: three tiles rotate (the shared output must outlive both branches).
//                        The weights are fragment-packed in consumption order per layer, [out tile][8 inputs][lane]
//                        float4 (element e of a lane: row lane & 31, input 8 c8 + 2 e + (lane >> 5)), behind the
//                        folded bias of every GEMM row. Thread n < 32 then finishes RoI n: (e) and (f).
// A column of the MFMA depends on no other column, so a slot's bits do not depend on which tile it sits in: the fused
// and the direct form agree bit for bit.
#include "dal3_block.h"
#include "dal3_kernels.h"
#include "dal3_roi_slots.h"

namespace {

constexpr int RH_BLOCK = 512, RH_WAVES = 8, RH_COLS = 32, RH_CK = 64, RH_SLD = 33, RH_MAXW = DAL3_ROI_MAX_WIDTH;
constexpr int RH_MAX_LAYERS = 11;

struct RoiLayer {
    int c_in, c_out, n_tiles, nc8, relu;
    int64_t bias_off, frag_off;          // in floats from the pack's start
};

struct RoiNet {
    int n_layers, n_shared, n_cls, n_reg, code;
    RoiLayer L[RH_MAX_LAYERS];
    int64_t floats;
};

// ---------------------------------------------------------------------------------- the points of a box
// point p of get_box_center: 0 the centre, 1 .. 4 the front, back, left, right mid-edges
__device__ __forceinline__ void box_point(const float* box, int cols, int p, float& x, float& y) {
    const float cx = box[0], cy = box[1];
    if (p == 0) {
        x = cx;
        y = cy;
        return;
    }
    const float dx = box[3], dy = box[4], a = box[cols - 1];
    const float s = sinf(a), c = cosf(a);
    const int ka = (p == 1 || p == 3) ? 0 : (p == 2 ? 2 : 1), kb = p == 1 ? 1 : (p == 4 ? 2 : 3);
    float px[2], py[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int k = i == 0 ? ka : kb;
        const float lx = __fmul_rn(dx, k >= 2 ? 0.5f : -0.5f), ly = __fmul_rn(dy, (k == 1 || k == 2) ? 0.5f : -0.5f);
        px[i] = __fadd_rn(__fadd_rn(__fmul_rn(lx, c), __fmul_rn(ly, s)), cx);
        py[i] = __fadd_rn(__fadd_rn(__fmul_rn(lx, -s), __fmul_rn(ly, c)), cy);
    }
    x = __fdiv_rn(__fadd_rn(px[0], px[1]), 2.0f);
    y = __fdiv_rn(__fadd_rn(py[0], py[1]), 2.0f);
}

__global__ __launch_bounds__(256) void box_points_kernel(const float* boxes, int64_t n, int cols, int P, float* out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * P; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i / n);
        const float* box = boxes + (i % n) * cols;
        float x, y;
        box_point(box, cols, p, x, y);
        out[i * 3 + 0] = x;
        out[i * 3 + 1] = y;
        out[i * 3 + 2] = box[2];
    }
}

// ---------------------------------------------------------------------------------- the gather
struct GatherGeom {
    int B, H, W, C, ppr, sample_index;
    const float* map;
    int64_t sb, sh, sw, sc;
    int64_t n;
    const float* xy;
    int64_t xy_stride;
    const int32_t* sample;
    float start[2], voxel[2], out_stride;
    float* out;
    int64_t row_stride, col_offset;
};

__global__ __launch_bounds__(256) void bev_gather_kernel(const GatherGeom g) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t i = wave; i < g.n; i += n_waves) {
        const int b = g.sample ? g.sample[i] : g.sample_index;
        if (b < 0 || b >= g.B) continue;
        const float x = __fdiv_rn(__fdiv_rn(__fsub_rn(g.xy[i * g.xy_stride], g.start[0]), g.voxel[0]), g.out_stride);
        const float y = __fdiv_rn(__fdiv_rn(__fsub_rn(g.xy[i * g.xy_stride + 1], g.start[1]), g.voxel[1]), g.out_stride);
        const float fx = floorf(x), fy = floorf(y), wm = (float)(g.W - 1), hm = (float)(g.H - 1);
        // fmaxf first: a NaN becomes 0; the clamp happens before the conversion, so every index lies inside the map
        const float x0 = fminf(fmaxf(fx, 0.f), wm), x1 = fminf(fmaxf(__fadd_rn(fx, 1.f), 0.f), wm);
        const float y0 = fminf(fmaxf(fy, 0.f), hm), y1 = fminf(fmaxf(__fadd_rn(fy, 1.f), 0.f), hm);
        const float ux = __fsub_rn(x1, x), lx = __fsub_rn(x, x0), uy = __fsub_rn(y1, y), ly = __fsub_rn(y, y0);
        const float wa = __fmul_rn(ux, uy), wb = __fmul_rn(ux, ly), wc = __fmul_rn(lx, uy), wd = __fmul_rn(lx, ly);
        const int64_t base = b * g.sb;
        const float* pa = g.map + base + (int64_t)y0 * g.sh + (int64_t)x0 * g.sw;
        const float* pb = g.map + base + (int64_t)y1 * g.sh + (int64_t)x0 * g.sw;
        const float* pc = g.map + base + (int64_t)y0 * g.sh + (int64_t)x1 * g.sw;
        const float* pd = g.map + base + (int64_t)y1 * g.sh + (int64_t)x1 * g.sw;
        float* o = g.out + (i / g.ppr) * g.row_stride + g.col_offset + (i % g.ppr) * g.C;
        for (int c = lane; c < g.C; c += 64) {
            const int64_t at = c * g.sc;
            float v = __fadd_rn(__fmul_rn(pa[at], wa), __fmul_rn(pb[at], wb));
            v = __fadd_rn(v, __fmul_rn(pc[at], wc));
            o[c] = __fadd_rn(v, __fmul_rn(pd[at], wd));
        }
    }
}

// ---------------------------------------------------------------------------------- the slots of the fused form
struct PrepareGeom {
    int B, M, T, P, cols;
    int64_t K, keep_stride;
    const float* boxes;
    const float* scores;
    const int32_t* labels;
    const int32_t* keep;
    const int32_t* keep_count;
    const int64_t* seg_offsets;
    int32_t label_base[DAL3_ROI_MAX_TASKS];
    float* rois;                         // (B, M, cols): rotation at column 6
    float* roi_scores;                   // (B, M)
    float* xy;                           // (B, M, P, 2)
    int32_t* sample;                     // (B, M, P)
    int32_t* out_labels;
    int32_t* counts;                     // (B): the workspace's
    int32_t* out_counts;
    int32_t* status;
};

__global__ __launch_bounds__(256) void roi_prepare_kernel(const PrepareGeom g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.B * g.M) return;
    const int b = (int)(i / g.M), m = (int)(i % g.M);
    int64_t before = 0, row = -1;
    int task = 0, bad = 0;
    roi_slot_row(g.keep, g.keep_count, g.seg_offsets, g.T, g.B, g.K, g.keep_stride, b, m, before, row, task, bad);
    if (m == 0) {
        const int32_t n = (int32_t)(before < g.M ? before : g.M);
        g.counts[b] = n;
        if (g.out_counts) g.out_counts[b] = n;
        if (before > g.M) atomicOr(g.status, DAL3_ROI_OVERFLOW);
    }
    if (bad) atomicOr(g.status, DAL3_NMS_BAD_SEGMENT);
    const bool live = row >= 0;
    for (int p = 0; p < g.P; ++p) g.sample[i * g.P + p] = live ? b : -1;
    if (!live) return;
    const float* box = g.boxes + row * g.cols;
    float* roi = g.rois + i * g.cols;
    for (int c = 0; c < 6; ++c) roi[c] = box[c];
    roi[6] = box[g.cols - 1];
    for (int c = 7; c < g.cols; ++c) roi[c] = box[c - 1];
    g.roi_scores[i] = g.scores[row];
    if (g.out_labels) g.out_labels[i] = g.labels[row] + g.label_base[task];
    for (int p = 0; p < g.P; ++p) {
        float x, y;
        box_point(box, g.cols, p, x, y);
        g.xy[(i * g.P + p) * 2] = x;
        g.xy[(i * g.P + p) * 2 + 1] = y;
    }
}

// ---------------------------------------------------------------------------------- the MLP
struct MlpGeom {
    RoiNet net;
    const float* packed;
    int B, M, PC, code;
    const int32_t* counts;               // (B) or NULL: every slot
    const float* rois;                   // (B, M, code)
    const float* roi_scores;             // (B, M)
    const float* features;               // (B, M, PC)
    float* out_boxes;
    float* out_scores;
    float* box_preds;
    float* cls_preds;
};

// steps (f): score and the rotation moved back to the last column
__device__ __forceinline__ void roi_post_row(const float* pred, float cls, float roi_score, int code, float* out_box, float* out_score) {
    if (out_score) *out_score = sqrtf(__fmul_rn(__fdiv_rn(1.f, __fadd_rn(1.f, expf(-cls))), roi_score));
    if (out_box) {
        for (int c = 0; c < 6; ++c) out_box[c] = pred[c];
        if (code == 9) {
            out_box[6] = pred[7];
            out_box[7] = pred[8];
            out_box[8] = pred[6];
        } else {
            out_box[6] = pred[6];
        }
    }
}

__global__ __launch_bounds__(256) void roi_post_kernel(const float* box_preds, const float* cls_preds, const float* roi_scores,
                                                       int64_t n, int code, float* out_boxes, float* out_scores) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        roi_post_row(box_preds + i * code, cls_preds[i], roi_scores[i], code, out_boxes ? out_boxes + i * code : nullptr,
                     out_scores ? out_scores + i : nullptr);
}

// one layer from an LDS tile [channel][32] to another
__device__ __forceinline__ void lds_layer(const RoiLayer& L, const float* __restrict__ packed, const float* in, float* out,
                                          int lane, int wave) {
    const int n = lane & 31, h = lane >> 5;
    const f32x4* frag = reinterpret_cast<const f32x4*>(packed + L.frag_off);
    for (int ot = wave; ot < L.n_tiles; ot += RH_WAVES) {
        f32x16 acc = tile_from_channels(packed + L.bias_off + 32 * ot, h);
        for (int c8 = 0; c8 < L.nc8; ++c8) {
            const f32x4 a = frag[((int64_t)ot * L.nc8 + c8) * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = mfma32(a[e], in[(8 * c8 + 2 * e + h) * RH_COLS + n], acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(32 * ot + tile_chan(r, h)) * RH_COLS + n] = L.relu ? relu1(acc[r]) : acc[r];
    }
}

__global__ __launch_bounds__(RH_BLOCK) void roi_mlp_kernel(const MlpGeom g) {
    __shared__ float act[3][RH_MAXW * RH_COLS];
    __shared__ float stage[RH_CK * RH_SLD];
    __shared__ float fin[2][32 * RH_COLS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int tiles_m = (g.M + RH_COLS - 1) / RH_COLS;
    const int b = blockIdx.x / tiles_m, m0 = (blockIdx.x % tiles_m) * RH_COLS;
    int count = g.counts ? g.counts[b] : g.M;
    if (count > g.M) count = g.M;
    if (m0 >= count) return;             // the whole workgroup: no barrier has been met
    const int64_t row0 = (int64_t)b * g.M + m0;
    const int live = count - m0 < RH_COLS ? count - m0 : RH_COLS;

    // ---- the first layer: one out tile per wave, the inputs staged 64 at a time
    {
        const RoiLayer& L = g.net.L[0];
        const f32x4* frag = reinterpret_cast<const f32x4*>(g.packed + L.frag_off);
        const bool mine = wave < L.n_tiles;
        f32x16 acc = mine ? tile_from_channels(g.packed + L.bias_off + 32 * wave, h) : f32x16{};
        const int n_chunks = (L.nc8 * 8 + RH_CK - 1) / RH_CK;
        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            __syncthreads();             // the previous chunk's reads are done
            const int c0 = chunk * RH_CK;
            for (int i = tid; i < RH_CK * RH_COLS; i += RH_BLOCK) {
                const int k = i % RH_CK, col = i / RH_CK;
                float v = 0.f;
                if (col < live && c0 + k < g.PC) v = g.features[(row0 + col) * g.PC + c0 + k];
                stage[k * RH_SLD + col] = v;
            }
            __syncthreads();
            if (mine) {
                f32x16 part = {};
#pragma unroll
                for (int k8 = 0; k8 < RH_CK / 8; ++k8) {
                    const int c8 = chunk * (RH_CK / 8) + k8;
                    if (c8 < L.nc8) {
                        const f32x4 a = frag[((int64_t)wave * L.nc8 + c8) * 64 + lane];
#pragma unroll
                        for (int e = 0; e < 4; ++e) part = mfma32(a[e], stage[(k8 * 8 + 2 * e + h) * RH_SLD + n], part);
                    }
                }
                acc += part;
            }
        }
        if (mine) {
#pragma unroll
            for (int r = 0; r < 16; ++r) act[0][(32 * wave + tile_chan(r, h)) * RH_COLS + n] = relu1(acc[r]);
        }
        __syncthreads();
    }
    // ---- the other shared layers
    int cur = 0, at = 1;
    for (; at < g.net.n_shared; ++at) {
        lds_layer(g.net.L[at], g.packed, act[cur], act[cur ^ 1], lane, wave);
        cur ^= 1;
        __syncthreads();
    }
    // ---- the two branches: hidden layers between the two free tiles, the final layer into fin[branch]
    for (int br = 0; br < 2; ++br) {
        const int hidden = br == 0 ? g.net.n_cls : g.net.n_reg;
        int in = cur, out = (cur + 1) % 3;
        for (int i = 0; i < hidden; ++i, ++at) {
            lds_layer(g.net.L[at], g.packed, act[in], act[out], lane, wave);
            __syncthreads();
            in = out;
            out = 3 - cur - in;          // the tile that is neither the shared output nor this layer's input
        }
        lds_layer(g.net.L[at], g.packed, act[in], fin[br], lane, wave);
        ++at;
        __syncthreads();
    }
    // ---- (e) and (f), one thread per RoI
    if (tid >= live) return;
    const int64_t row = row0 + tid;
    const float* roi = g.rois + row * g.code;
    float pred[9];
    for (int c = 0; c < g.code; ++c) pred[c] = __fadd_rn(fin[1][c * RH_COLS + tid], c < 3 ? 0.f : roi[c]);
    const float s = sinf(roi[6]), c = cosf(roi[6]);
    const float x = __fadd_rn(__fmul_rn(pred[0], c), __fmul_rn(pred[1], s));
    const float y = __fadd_rn(__fmul_rn(pred[0], -s), __fmul_rn(pred[1], c));
    pred[0] = __fadd_rn(x, roi[0]);
    pred[1] = __fadd_rn(y, roi[1]);
    pred[2] = __fadd_rn(pred[2], roi[2]);
    const float cls = fin[0][tid];
    if (g.box_preds) {
        for (int k = 0; k < g.code; ++k) g.box_preds[row * g.code + k] = pred[k];
    }
    if (g.cls_preds) g.cls_preds[row] = cls;
    roi_post_row(pred, cls, g.roi_scores[row], g.code, g.out_boxes ? g.out_boxes + row * g.code : nullptr,
                 g.out_scores ? g.out_scores + row : nullptr);
}

bool width_ok(int w) { return w >= 16 && w <= RH_MAXW && w % 16 == 0; }

// the network of a shape -> false when it is not served. A layer's section of the pack, [bias_off, next bias_off), IS
// dal3_conv2d_pack's blob of a DAL3_CONV2D_1X1 layer of the same (c_in, c_out): conv2d_pack_floats(1X1, c_in, c_out)
// floats, the n_tiles * 32 folded biases and then the [out tile][8 inputs][lane] float4 fragments at frag_off
bool roi_net(const dal3_roi_shape& s, RoiNet& net) {
    net = RoiNet{};
    if (s.c_in < 1 || s.c_in > 5 * 65535 || s.num_class != 1 || (s.code_size != 7 && s.code_size != 9)) return false;
    if (s.n_shared < 1 || s.n_shared > 3 || s.n_cls < 1 || s.n_cls > 3 || s.n_reg < 1 || s.n_reg > 3) return false;
    int64_t off = 0;
    int n = 0, c_in = s.c_in;
    auto add = [&](int c_out, int relu) {
        RoiLayer& L = net.L[n++];
        L.c_in = c_in;
        L.c_out = c_out;
        L.n_tiles = (c_out + 31) / 32;
        L.nc8 = (c_in + 7) / 8;
        L.relu = relu;
        L.bias_off = off;
        L.frag_off = off + (int64_t)L.n_tiles * 32;
        off = L.frag_off + (int64_t)L.n_tiles * L.nc8 * 256;
        c_in = c_out;
    };
    for (int i = 0; i < s.n_shared; ++i) {
        if (!width_ok(s.shared[i])) return false;
        add(s.shared[i], 1);
    }
    const int shared_out = c_in;
    for (int i = 0; i < s.n_cls; ++i) {
        if (!width_ok(s.cls[i])) return false;
        add(s.cls[i], 1);
    }
    add(s.num_class, 0);
    c_in = shared_out;
    for (int i = 0; i < s.n_reg; ++i) {
        if (!width_ok(s.reg[i])) return false;
        add(s.reg[i], 1);
    }
    add(s.code_size, 0);
    net.n_layers = n;
    net.n_shared = s.n_shared, net.n_cls = s.n_cls, net.n_reg = s.n_reg, net.code = s.code_size;
    net.floats = off;
    return true;
}

struct RoiWorkspace {
    float *rois, *roi_scores, *xy, *features;
    int32_t *sample, *counts;
};

RoiWorkspace carve_roi(Carver& c, int64_t B, int64_t M, int P, int C, int code) {
    RoiWorkspace w;
    const size_t rows = (size_t)(B * M);
    w.rois = c.take<float>(rows * code);
    w.roi_scores = c.take<float>(rows);
    w.xy = c.take<float>(rows * P * 2);
    w.sample = c.take<int32_t>(rows * P);
    w.counts = c.take<int32_t>((size_t)B);
    w.features = c.take<float>(rows * P * C);
    return w;
}

unsigned blocks_for(int64_t n, int per) {
    int64_t b = (n + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b));
}

}  // namespace

hipError_t launch_bev_gather(const dal3_bev_gather_args* a, hipStream_t s) {
    if (a->n <= 0) return hipSuccess;
    GatherGeom g = {};
    g.B = (int)a->B, g.H = (int)a->H, g.W = (int)a->W, g.C = a->C, g.ppr = a->points_per_row, g.sample_index = a->sample_index;
    g.map = a->map.data;
    g.sb = a->map.stride_b, g.sh = a->map.stride_h, g.sw = a->map.stride_w, g.sc = a->map.stride_c;
    g.n = a->n, g.xy = a->xy, g.xy_stride = a->xy_stride, g.sample = a->sample;
    g.start[0] = a->pc_start[0], g.start[1] = a->pc_start[1], g.voxel[0] = a->voxel_size[0], g.voxel[1] = a->voxel_size[1];
    g.out_stride = a->out_stride;
    g.out = a->out, g.row_stride = a->out_row_stride, g.col_offset = a->out_col_offset;
    hipLaunchKernelGGL(bev_gather_kernel, dim3(blocks_for(a->n, 4)), dim3(256), 0, s, g);
    return hipGetLastError();
}

hipError_t launch_box_points(const float* boxes, int64_t n, int cols, int num_point, float* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(box_points_kernel, dim3(blocks_for(n * num_point, 256)), dim3(256), 0, s, boxes, n, cols, num_point, out);
    return hipGetLastError();
}

size_t roi_pack_floats(const dal3_roi_shape* shape) {
    RoiNet net;
    return roi_net(*shape, net) ? (size_t)net.floats : 0;
}

int roi_layers(const dal3_roi_shape* shape) {
    RoiNet net;
    return roi_net(*shape, net) ? net.n_layers : 0;
}

// layer i's (c_in, c_out) of a served shape
void roi_layer_dims(const dal3_roi_shape* shape, int i, int* c_in, int* c_out) {
    RoiNet net;
    roi_net(*shape, net);
    *c_in = net.L[i].c_in;
    *c_out = net.L[i].c_out;
}

// every section is the dense stage's 1x1 pack of its layer (roi_net), written by that packer with the layer's own eps
hipError_t launch_roi_pack(const dal3_roi_shape* shape, const dal3_layer* layers, const double* eps, float* out, hipStream_t s) {
    RoiNet net;
    roi_net(*shape, net);
    for (int i = 0; i < net.n_layers; ++i) {
        const hipError_t e = launch_conv2d_pack(FoldLayer(layers[i], eps ? eps[i] : 1e-5), DAL3_CONV2D_1X1, out + net.L[i].bias_off, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

size_t roi_head_workspace_bytes(int64_t B, int64_t M, int num_point, int C, int code_size) {
    Carver c(nullptr, 0);
    carve_roi(c, B, M, num_point, C, code_size);
    return c.off;
}

hipError_t launch_roi_post(const float* box_preds, const float* cls_preds, const float* roi_scores, int64_t n, int code_size,
                           float* out_boxes, float* out_scores, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(roi_post_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, box_preds, cls_preds, roi_scores, n, code_size,
                       out_boxes, out_scores);
    return hipGetLastError();
}

// the arguments are checked by dal3_api.hip; false: the workspace is too small
bool launch_roi_head(const dal3_roi_head_args* args, hipStream_t s, hipError_t* err) {
    const dal3_roi_head_args& a = *args;
    *err = hipSuccess;
    if (a.B <= 0 || a.M <= 0) return true;
    const int P = a.num_point, code = a.shape.code_size;
    MlpGeom g = {};
    roi_net(a.shape, g.net);
    g.packed = a.packed;
    g.B = (int)a.B, g.M = (int)a.M, g.PC = a.shape.c_in, g.code = code;
    g.out_boxes = a.out_boxes, g.out_scores = a.out_scores, g.box_preds = a.box_preds, g.cls_preds = a.cls_preds;
    if (a.keep) {
        Carver c(a.workspace, a.workspace_bytes);
        const RoiWorkspace w = carve_roi(c, a.B, a.M, P, a.C, code);
        if (!c.ok) return false;
        PrepareGeom p = {};
        p.B = (int)a.B, p.M = (int)a.M, p.T = a.T, p.P = P, p.cols = a.box_cols;
        p.K = a.K, p.keep_stride = a.keep_stride;
        p.boxes = a.boxes, p.scores = a.scores, p.labels = a.labels, p.keep = a.keep, p.keep_count = a.keep_count;
        p.seg_offsets = a.seg_offsets;
        for (int t = 0; t < DAL3_ROI_MAX_TASKS; ++t) p.label_base[t] = a.label_base[t];
        p.rois = w.rois, p.roi_scores = w.roi_scores, p.xy = w.xy, p.sample = w.sample;
        p.out_labels = a.out_labels, p.counts = w.counts, p.out_counts = a.out_counts, p.status = a.status;
        hipLaunchKernelGGL(roi_prepare_kernel, dim3(blocks_for(a.B * a.M, 256)), dim3(256), 0, s, p);
        if ((*err = hipGetLastError()) != hipSuccess) return true;
        float* features = a.out_features ? a.out_features : w.features;
        dal3_bev_gather_args ga = {};
        ga.B = a.B, ga.H = a.H, ga.W = a.W, ga.C = a.C, ga.map = a.bev;
        ga.n = a.B * a.M * P, ga.xy = w.xy, ga.xy_stride = 2, ga.sample = w.sample;
        ga.pc_start[0] = a.pc_start[0], ga.pc_start[1] = a.pc_start[1];
        ga.voxel_size[0] = a.voxel_size[0], ga.voxel_size[1] = a.voxel_size[1], ga.out_stride = a.out_stride;
        ga.points_per_row = P, ga.out = features, ga.out_row_stride = (int64_t)P * a.C, ga.out_col_offset = 0;
        if ((*err = launch_bev_gather(&ga, s)) != hipSuccess) return true;
        g.counts = w.counts, g.rois = w.rois, g.roi_scores = w.roi_scores, g.features = features;
    } else {
        g.counts = nullptr, g.rois = a.rois, g.roi_scores = a.roi_scores, g.features = a.roi_features;
    }
    const int64_t tiles = a.B * ((a.M + RH_COLS - 1) / RH_COLS);
    hipLaunchKernelGGL(roi_mlp_kernel, dim3((unsigned)tiles), dim3(RH_BLOCK), 0, s, g);
    *err = hipGetLastError();
    return true;
}
