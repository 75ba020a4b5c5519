// dal3_conv2d_train.hip — the backward pass of the detector's dense stage (dal3_conv2d_dgrad_pack / dal3_conv2d_dgrad /
// dal3_conv2d_wgrad of include/dal3.h), float32 on v_mfma_f32_32x32x2_f32. Built with IEEE NaN semantics: a diverged loss
// must reach the gradients.
//
// dgrad serves the three forms whose data gradient is no forward form (3x3 stride 1 and 1x1 are dal3_conv2d on dy with
// the transposed pack). It is the implicit-GEMM body of dal3_conv2d.hip in the same orientation: dx channels (GEMM rows)
// on the MFMA rows, 32 pixels of one row on its columns (= lanes), two contraction channels per k-step.
//   3x3 stride 2: by the parity of (iy, ix) dx falls into four phases; pixel (2 m + py, 2 n + px) of phase (py, px) sums
//     the taps ky in {1} (py = 0) or {2, 0} (py = 1), which read dy row m, or m and m + 1, and the same along x: 1, 2, 2
//     and 4 taps. A workgroup's pixel grid is one phase's sub-grid, so the reads of dy are unit-stride and the store has
//     stride 2; the phase is part of the work index and only the taps that are present are multiplied.
//   k = s transposed convolutions: the 1x1 form with K = c_out * s * s (k = (co * s + dy) * s + dx, the weight's own
//     (c_in, K) layout) and a pixel-unshuffle load of dy in the staging loop.
//
// wgrad is a GEMM with the pixels as the contraction: the channels of one map ("A": dy, or x for a transposed convolution)
// on the MFMA rows, the channels of the other ("B": x, or dy) on its columns, lane half h supplies pixel 2 t + h of k-step
// t. A workgroup owns (32 A channels, 32 B channels, one kernel row ky, one slice of pixel tiles) and keeps one
// accumulator per kx; a pixel tile is 4 rows (one per wave) x TC columns, staged in LDS pixel-major with the channel
// fastest (row length 33: the staging writes walk pixels, the operand reads walk channels, both without a bank
// conflict), B with its TC * S + KW - S columns of the row ky selects, zero outside the image. At the end of its slice
// the four waves' accumulators are added in LDS in wave order and the partial goes to the workspace; a second kernel
// adds the slices in ascending order. The order of every sum is a function of the shapes alone.
#include "dal3_kernels.h"

namespace {

constexpr int CT_BLOCK = 256;

// ---------------------------------------------------------------------------------------------------------------- dgrad
constexpr int DG_ROWS = 8, DG_COLS = 32, DG_CK = 16;

// fragments [dx tile][8 contraction channels][tap][lane] float4: element e of a lane is row lane & 31, channel
// 8 c8 + 2 e + (lane >> 5). 3x3: W[k][row][tap] of the (c_out, c_in, 3, 3) weight; deconv: W[row][k] of (c_in, c_out * s * s).
__global__ __launch_bounds__(CT_BLOCK) void dgrad_pack_kernel(const float* __restrict__ w, int deconv, int c_in, int K, int nk8,
                                                              int64_t total, float* __restrict__ out) {
    const int taps = deconv ? 1 : 9;
    for (int64_t i = (int64_t)blockIdx.x * CT_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * CT_BLOCK) {
        const int e = (int)(i & 3), lane = (int)((i >> 2) & 63);
        const int64_t t = i >> 8;
        const int tap = (int)(t % taps), c8 = (int)((t / taps) % nk8), ot = (int)(t / ((int64_t)taps * nk8));
        const int row = 32 * ot + (lane & 31), k = 8 * c8 + 2 * e + (lane >> 5);
        float v = 0.f;
        if (row < c_in && k < K) v = deconv ? w[(int64_t)row * K + k] : w[((int64_t)k * c_in + row) * 9 + tap];
        out[i] = v;
    }
}

struct DgradGeom {
    int c_in, c_out, K, s, nk8, n_groups;    // GEMM rows = c_in; K = the contraction's channels; s: the deconv's (else 2)
    int H, W, GH, GW;                        // dx's extent; dy's extent
    int tiles_y, tiles_x, n_phase;
    int64_t n_work;                          // B * n_phase * tiles_y * tiles_x * n_groups
    const float* dy;
    int64_t gb, gh, gw, gc;
    float* dx;
    int64_t xb, xh, xw, xc;
    const f32x4* frag;
};

template <bool DECONV, int MT>
__global__ __launch_bounds__(CT_BLOCK, 2) void dgrad_kernel(const DgradGeom g) {
    constexpr int TAPS = DECONV ? 1 : 9, T = 2;
    constexpr int IR = DECONV ? DG_ROWS : DG_ROWS + 1, PW = DECONV ? DG_COLS : DG_COLS + 1, PS = IR * PW;
    __shared__ float tile[DG_CK * PS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int n_chunks = (g.nk8 * 8 + DG_CK - 1) / DG_CK;
    const int lds0 = h * PS + (wave * T) * PW + n;
    const int ss = g.s * g.s;

    for (int64_t work = blockIdx.x; work < g.n_work; work += gridDim.x) {
        const int grp = (int)(work % g.n_groups);
        int64_t rest = work / g.n_groups;
        const int tx = (int)(rest % g.tiles_x);
        rest /= g.tiles_x;
        const int ty = (int)(rest % g.tiles_y);
        rest /= g.tiles_y;
        const int phase = (int)(rest % g.n_phase), b = (int)(rest / g.n_phase);
        const int py = DECONV ? 0 : phase >> 1, px = DECONV ? 0 : phase & 1;
        const int m0 = ty * DG_ROWS, n0 = tx * DG_COLS;
        // the phase's sub-grid: the pixels (2 m + py, 2 n + px) inside dx
        const int sub_h = DECONV ? g.H : (g.H - py + 1) / 2, sub_w = DECONV ? g.W : (g.W - px + 1) / 2;
        if (m0 >= sub_h || n0 >= sub_w) continue;              // workgroup-uniform
        const int nty = py ? 2 : 1, ntx = px ? 2 : 1;
        const int ot0 = grp * MT;

        f32x16 acc[MT][T];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int j = 0; j < T; ++j) acc[mt][j] = f32x16{};
        }

        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            __syncthreads();
            const int c0 = chunk * DG_CK;
            for (int i = tid; i < DG_CK * PS; i += CT_BLOCK) {
                const int c = i / PS, rem = i % PS, r = rem / PW, col = rem % PW;
                const int k = c0 + c;
                float v = 0.f;
                if (DECONV) {
                    const int y = m0 + r, x = n0 + col;
                    if (k < g.K && y < g.H && x < g.W) {
                        const int co = k / ss, dd = k % ss;
                        v = g.dy[b * g.gb + co * g.gc + (int64_t)(y * g.s + dd / g.s) * g.gh + (int64_t)(x * g.s + dd % g.s) * g.gw];
                    }
                } else {
                    const int oy = m0 + r, ox = n0 + col;
                    if (k < g.K && oy < g.GH && ox < g.GW) v = g.dy[b * g.gb + k * g.gc + oy * g.gh + ox * g.gw];
                }
                tile[i] = v;
            }
            __syncthreads();
            // as in the forward kernel, a chunk's terms are summed from zero and then added to the total
            f32x16 part[MT][T];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < T; ++j) part[mt][j] = f32x16{};
            }
#pragma unroll
            for (int k8 = 0; k8 < DG_CK / 8; ++k8) {
                const int c8 = chunk * (DG_CK / 8) + k8;
                if (c8 >= g.nk8) continue;
                for (int ty_ = 0; ty_ < nty; ++ty_) {
                    for (int tx_ = 0; tx_ < ntx; ++tx_) {
                        // py = 0: tap 1 reads dy row m. py = 1: tap 2 reads row m, tap 0 row m + 1. The same along x.
                        const int ky = py ? (ty_ ? 0 : 2) : 1, kx = px ? (tx_ ? 0 : 2) : 1;
                        const int tap = DECONV ? 0 : ky * 3 + kx;
                        const int at = ty_ * PW + tx_;
                        f32x4 a[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            a[mt] = g.frag[(((int64_t)(ot0 + mt) * g.nk8 + c8) * TAPS + tap) * 64 + lane];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float bv[T];
#pragma unroll
                            for (int j = 0; j < T; ++j) bv[j] = tile[lds0 + (k8 * 8 + 2 * e) * PS + j * PW + at];
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                                for (int j = 0; j < T; ++j) part[mt][j] = mfma32(a[mt][e], bv[j], part[mt][j]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < T; ++j) acc[mt][j] += part[mt][j];
            }
        }

        const int ix = DECONV ? n0 + n : 2 * (n0 + n) + px;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const int m = m0 + wave * T + j, iy = DECONV ? m : 2 * m + py;
                if (iy >= g.H || ix >= g.W) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * (ot0 + mt) + tile_chan(r, h);
                    if (row >= g.c_in) continue;
                    g.dx[b * g.xb + row * g.xc + iy * g.xh + ix * g.xw] = acc[mt][j][r];
                }
            }
        }
    }
}

template <bool DECONV>
void launch_dgrad_mt(const DgradGeom& g, int mt, dim3 grid, hipStream_t s) {
    if (mt == 2) hipLaunchKernelGGL((dgrad_kernel<DECONV, 2>), grid, dim3(CT_BLOCK), 0, s, g);
    else hipLaunchKernelGGL((dgrad_kernel<DECONV, 1>), grid, dim3(CT_BLOCK), 0, s, g);
}

// ---------------------------------------------------------------------------------------------------------------- wgrad
constexpr int WG_TR = 4, WG_LD = 33;

struct WgradGeom {
    int CA, CB;                              // channels of the A map (MFMA rows) and of the B map (MFMA columns)
    int PH, PW, BH, BW;                      // the pixel grid (A's extent); B's extent
    int n_at, n_bt, KH;                      // tiles of 32 A / B channels; kernel rows
    int tiles_y, tiles_x, tiles_per_slice, n_slices;
    int64_t n_ptiles, n_work;                // B * tiles_y * tiles_x; n_at * n_bt * KH * n_slices
    int64_t sA, sB, dw_elems;                // dw element (row, col, ky, kx) = row * sA + col * sB + ky * KW + kx
    const float* a;
    int64_t ab, ah, aw, ac;
    const float* b;
    int64_t bb, bh, bw, bc;
    float* ws;                               // (n_slices, dw_elems)
};

template <int KW, int S, int PAD, int TC>
__global__ __launch_bounds__(CT_BLOCK) void wgrad_kernel(const WgradGeom g) {
    constexpr int IC = (TC - 1) * S + KW;
    constexpr int NA = WG_TR * TC * WG_LD, NB = WG_TR * IC * WG_LD;
    constexpr int NL = NA + NB > 4096 ? NA + NB : 4096;
    __shared__ float lds[NL];
    float* const la = lds;
    float* const lb = lds + NA;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;

    for (int64_t work = blockIdx.x; work < g.n_work; work += gridDim.x) {
        const int slice = (int)(work % g.n_slices);
        int64_t rest = work / g.n_slices;
        const int ky = (int)(rest % g.KH);
        rest /= g.KH;
        const int bt = (int)(rest % g.n_bt), at = (int)(rest / g.n_bt);

        f32x16 acc[KW];
#pragma unroll
        for (int kx = 0; kx < KW; ++kx) acc[kx] = f32x16{};

        const int64_t pt0 = (int64_t)slice * g.tiles_per_slice;
        const int64_t pt1 = pt0 + g.tiles_per_slice < g.n_ptiles ? pt0 + g.tiles_per_slice : g.n_ptiles;
        for (int64_t pt = pt0; pt < pt1; ++pt) {
            const int tx = (int)(pt % g.tiles_x);
            const int64_t rr = pt / g.tiles_x;
            const int ty = (int)(rr % g.tiles_y), b = (int)(rr / g.tiles_y);
            const int py0 = ty * WG_TR, px0 = tx * TC;
            __syncthreads();                                   // the previous tile's (or the reduction's) reads are done
            for (int i = tid; i < 32 * WG_TR * TC; i += CT_BLOCK) {
                const int ch = i / (WG_TR * TC), p = i % (WG_TR * TC), y = py0 + p / TC, x = px0 + p % TC, c = at * 32 + ch;
                float v = 0.f;
                if (c < g.CA && y < g.PH && x < g.PW) v = g.a[b * g.ab + c * g.ac + y * g.ah + x * g.aw];
                la[p * WG_LD + ch] = v;
            }
            for (int i = tid; i < 32 * WG_TR * IC; i += CT_BLOCK) {
                const int ch = i / (WG_TR * IC), p = i % (WG_TR * IC), c = bt * 32 + ch;
                const int y = (py0 + p / IC) * S + ky - PAD, x = px0 * S - PAD + p % IC;
                float v = 0.f;
                if (c < g.CB && y >= 0 && y < g.BH && x >= 0 && x < g.BW) v = g.b[b * g.bb + c * g.bc + y * g.bh + x * g.bw];
                lb[p * WG_LD + ch] = v;
            }
            __syncthreads();
#pragma unroll 4
            for (int t = 0; t < TC / 2; ++t) {
                const int col = 2 * t + h;
                const float av = la[(wave * TC + col) * WG_LD + n];
#pragma unroll
                for (int kx = 0; kx < KW; ++kx) acc[kx] = mfma32(av, lb[(wave * IC + col * S + kx) * WG_LD + n], acc[kx]);
            }
        }

        // the four waves' sums in wave order, then the slice's partial in the parameter's own layout
#pragma unroll
        for (int kx = 0; kx < KW; ++kx) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) lds[wave * 1024 + r * 64 + lane] = acc[kx][r];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = tid + CT_BLOCK * q, r = idx >> 6, l = idx & 63;
                const float v = ((lds[idx] + lds[1024 + idx]) + lds[2048 + idx]) + lds[3072 + idx];
                const int row = at * 32 + tile_chan(r, l >> 5), col = bt * 32 + (l & 31);
                if (row < g.CA && col < g.CB) g.ws[slice * g.dw_elems + row * g.sA + col * g.sB + ky * KW + kx] = v;
            }
        }
    }
}

// dw[i] = the slices' partials in ascending slice order
__global__ __launch_bounds__(CT_BLOCK) void wgrad_sum_kernel(const float* __restrict__ ws, int n_slices, int64_t n, float* __restrict__ dw) {
    for (int64_t i = (int64_t)blockIdx.x * CT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CT_BLOCK) {
        float v = 0.f;
        for (int s = 0; s < n_slices; ++s) v += ws[s * n + i];
        dw[i] = v;
    }
}

// db[c] = the sum of channel c of dy: the workgroup is 8 rows x 32 columns of threads, thread (ly, lx) adds the pixels
// (row ly + 8 i of the B * H rows, column lx + 32 j) in that order, then a fixed tree.
// Summed in float64 and rounded once: db of the head's final layers is a vector of one to three elements, where nothing
// averages a float32 chain's rounding out, and the adds are a negligible part of the pass.
__global__ __launch_bounds__(CT_BLOCK) void bias_grad_kernel(const float* __restrict__ dy, int64_t sb, int64_t sh, int64_t sw, int64_t sc,
                                                             int C, int H, int W, int64_t n_rows, float* __restrict__ db) {
    __shared__ double red[CT_BLOCK];
    const int tid = threadIdx.x, lx = tid & 31, ly = tid >> 5;
    for (int c = blockIdx.x; c < C; c += gridDim.x) {
        double v = 0.0;
        for (int64_t q = ly; q < n_rows; q += CT_BLOCK / 32) {
            const float* row = dy + (q / H) * sb + c * sc + (q % H) * sh;
#pragma unroll 4
            for (int x = lx; x < W; x += 32) v += row[x * sw];
        }
        __syncthreads();
        red[tid] = v;
        __syncthreads();
        for (int step = CT_BLOCK / 2; step > 0; step >>= 1) {
            if (tid < step) red[tid] += red[tid + step];
            __syncthreads();
        }
        if (tid == 0) db[c] = (float)red[0];
    }
}

struct WgradPlan {
    int tc, tiles_y, tiles_x, tiles_per_slice, n_slices;
    int64_t n_ptiles, dw_elems;
};

WgradPlan wgrad_plan(int kind, int stride, int c_in, int c_out, int64_t B, int64_t H, int64_t W) {
    WgradPlan p = {};
    const bool deconv = kind == DAL3_CONV2D_DECONV2 || kind == DAL3_CONV2D_DECONV4;
    const int cs = kind == DAL3_CONV2D_3X3 ? stride : 1;
    const int64_t PH = H > 0 ? (H - 1) / cs + 1 : 0, PW = W > 0 ? (W - 1) / cs + 1 : 0;
    p.tc = kind == DAL3_CONV2D_DECONV4 ? 16 : 32;
    p.tiles_y = (int)((PH + WG_TR - 1) / WG_TR);
    p.tiles_x = (int)((PW + p.tc - 1) / p.tc);
    p.n_ptiles = B * p.tiles_y * p.tiles_x;
    p.tiles_per_slice = DAL3_CONV2D_WGRAD_SLICE / (WG_TR * p.tc);
    p.n_slices = (int)((p.n_ptiles + p.tiles_per_slice - 1) / p.tiles_per_slice);
    p.dw_elems = (int64_t)c_in * c_out * (kind == DAL3_CONV2D_3X3 ? 9 : deconv ? stride * stride : 1);
    return p;
}

}  // namespace

size_t conv2d_dgrad_pack_floats(int kind, int c_in, int c_out) {
    const int64_t K = kind == DAL3_CONV2D_3X3 ? c_out : (int64_t)c_out * (kind == DAL3_CONV2D_DECONV2 ? 4 : 16);
    const int64_t n_tiles = (c_in + 31) / 32, nk8 = (K + 7) / 8;
    return (size_t)(n_tiles * nk8 * (kind == DAL3_CONV2D_3X3 ? 9 : 1) * 256);
}

hipError_t launch_conv2d_dgrad_pack(const float* weight, int kind, int c_in, int c_out, float* out, hipStream_t s) {
    const int deconv = kind != DAL3_CONV2D_3X3;
    const int K = deconv ? c_out * (kind == DAL3_CONV2D_DECONV2 ? 4 : 16) : c_out;
    const int64_t total = (int64_t)conv2d_dgrad_pack_floats(kind, c_in, c_out);
    int64_t blocks = (total + CT_BLOCK - 1) / CT_BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(dgrad_pack_kernel, dim3((unsigned)blocks), dim3(CT_BLOCK), 0, s, weight, deconv, c_in, K, (K + 7) / 8, total, out);
    return hipGetLastError();
}

hipError_t launch_conv2d_dgrad(const dal3_conv2d_dgrad_args* args, hipStream_t s) {
    const dal3_conv2d_dgrad_args& a = *args;
    if (a.B <= 0 || a.H <= 0 || a.W <= 0) return hipSuccess;
    const bool deconv = a.kind != DAL3_CONV2D_3X3;
    DgradGeom g = {};
    g.c_in = a.c_in, g.c_out = a.c_out;
    g.s = a.stride;
    g.K = deconv ? a.c_out * a.stride * a.stride : a.c_out;
    g.nk8 = (g.K + 7) / 8;
    const int n_tiles = (a.c_in + 31) / 32, mt = n_tiles % 2 == 0 ? 2 : 1;
    g.n_groups = n_tiles / mt;
    g.H = (int)a.H, g.W = (int)a.W;
    g.GH = deconv ? g.H * a.stride : (g.H - 1) / 2 + 1;
    g.GW = deconv ? g.W * a.stride : (g.W - 1) / 2 + 1;
    g.n_phase = deconv ? 1 : 4;
    const int sub_h = deconv ? g.H : (g.H + 1) / 2, sub_w = deconv ? g.W : (g.W + 1) / 2;
    g.tiles_y = (sub_h + DG_ROWS - 1) / DG_ROWS;
    g.tiles_x = (sub_w + DG_COLS - 1) / DG_COLS;
    g.n_work = a.B * g.n_phase * g.tiles_y * g.tiles_x * g.n_groups;
    g.dy = a.dy.data;
    g.gb = a.dy.stride_b, g.gh = a.dy.stride_h, g.gw = a.dy.stride_w, g.gc = a.dy.stride_c;
    g.dx = const_cast<float*>(a.dx.data);
    g.xb = a.dx.stride_b, g.xh = a.dx.stride_h, g.xw = a.dx.stride_w, g.xc = a.dx.stride_c;
    g.frag = reinterpret_cast<const f32x4*>(a.packed);
    int64_t blocks = g.n_work;
    if (a.max_workgroups > 0 && blocks > a.max_workgroups) blocks = a.max_workgroups;
    if (blocks > 0x7fffffff) blocks = 0x7fffffff;
    if (deconv) launch_dgrad_mt<true>(g, mt, dim3((unsigned)blocks), s);
    else launch_dgrad_mt<false>(g, mt, dim3((unsigned)blocks), s);
    return hipGetLastError();
}

size_t conv2d_wgrad_workspace_bytes(int kind, int stride, int c_in, int c_out, int64_t B, int64_t H, int64_t W) {
    const WgradPlan p = wgrad_plan(kind, stride, c_in, c_out, B, H, W);
    return (size_t)p.n_slices * (size_t)p.dw_elems * sizeof(float);
}

hipError_t launch_conv2d_wgrad(const dal3_conv2d_wgrad_args* args, hipStream_t s) {
    const dal3_conv2d_wgrad_args& a = *args;
    const bool deconv = a.kind == DAL3_CONV2D_DECONV2 || a.kind == DAL3_CONV2D_DECONV4;
    const WgradPlan p = wgrad_plan(a.kind, a.stride, a.c_in, a.c_out, a.B, a.H, a.W);
    const int cs = a.kind == DAL3_CONV2D_3X3 ? a.stride : 1;
    const int OH = a.H > 0 ? (int)((a.H - 1) / cs + 1) * (deconv ? a.stride : 1) : 0;
    const int OW = a.W > 0 ? (int)((a.W - 1) / cs + 1) * (deconv ? a.stride : 1) : 0;
    const int cap = a.max_workgroups;
    if (p.n_ptiles > 0) {
        WgradGeom g = {};
        const dal3_map& ma = deconv ? a.x : a.dy;
        const dal3_map& mb = deconv ? a.dy : a.x;
        g.CA = deconv ? a.c_in : a.c_out, g.CB = deconv ? a.c_out : a.c_in;
        g.PH = deconv ? (int)a.H : OH, g.PW = deconv ? (int)a.W : OW;
        g.BH = deconv ? OH : (int)a.H, g.BW = deconv ? OW : (int)a.W;
        g.n_at = (g.CA + 31) / 32, g.n_bt = (g.CB + 31) / 32;
        g.KH = a.kind == DAL3_CONV2D_3X3 ? 3 : deconv ? a.stride : 1;
        g.tiles_y = p.tiles_y, g.tiles_x = p.tiles_x, g.tiles_per_slice = p.tiles_per_slice, g.n_slices = p.n_slices;
        g.n_ptiles = p.n_ptiles;
        g.n_work = (int64_t)g.n_at * g.n_bt * g.KH * g.n_slices;
        const int64_t taps = (int64_t)g.KH * g.KH;
        g.sA = g.CB * taps, g.sB = taps, g.dw_elems = p.dw_elems;
        g.a = ma.data, g.ab = ma.stride_b, g.ah = ma.stride_h, g.aw = ma.stride_w, g.ac = ma.stride_c;
        g.b = mb.data, g.bb = mb.stride_b, g.bh = mb.stride_h, g.bw = mb.stride_w, g.bc = mb.stride_c;
        g.ws = static_cast<float*>(a.workspace);
        int64_t blocks = g.n_work;
        if (cap > 0 && blocks > cap) blocks = cap;
        if (blocks > 0x7fffffff) blocks = 0x7fffffff;
        const dim3 grid((unsigned)blocks), block(CT_BLOCK);
        if (a.kind == DAL3_CONV2D_3X3 && a.stride == 1) hipLaunchKernelGGL((wgrad_kernel<3, 1, 1, 32>), grid, block, 0, s, g);
        else if (a.kind == DAL3_CONV2D_3X3) hipLaunchKernelGGL((wgrad_kernel<3, 2, 1, 32>), grid, block, 0, s, g);
        else if (a.kind == DAL3_CONV2D_1X1) hipLaunchKernelGGL((wgrad_kernel<1, 1, 0, 32>), grid, block, 0, s, g);
        else if (a.kind == DAL3_CONV2D_DECONV2) hipLaunchKernelGGL((wgrad_kernel<2, 2, 0, 32>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((wgrad_kernel<4, 4, 0, 16>), grid, block, 0, s, g);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    int64_t blocks = (p.dw_elems + CT_BLOCK - 1) / CT_BLOCK;
    if (blocks > 4096) blocks = 4096;
    if (cap > 0 && blocks > cap) blocks = cap;
    hipLaunchKernelGGL(wgrad_sum_kernel, dim3((unsigned)blocks), dim3(CT_BLOCK), 0, s, static_cast<const float*>(a.workspace), p.n_slices,
                       p.dw_elems, a.dw);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.db) return e;
    blocks = a.c_out;
    if (cap > 0 && blocks > cap) blocks = cap;
    hipLaunchKernelGGL(bias_grad_kernel, dim3((unsigned)blocks), dim3(CT_BLOCK), 0, s, a.dy.data, a.dy.stride_b, a.dy.stride_h,
                       a.dy.stride_w, a.dy.stride_c, a.c_out, OH, OW, a.B * (int64_t)OH, a.db);
    return hipGetLastError();
}
