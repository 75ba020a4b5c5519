// dal3_conv2d.hip — the detector's dense stage (dal3_conv2d_pack / dal3_conv2d of include/dal3.h): the 3x3 and 1x1
// convolutions and the k = s transposed convolutions of the RPN neck and the CenterHead, as ONE implicit-GEMM body on
// v_mfma_f32_32x32x2_f32 in the orientation of dal3_device.h: output channels (GEMM rows) on the MFMA rows, 32 output
// pixels of one image row on its columns (= lanes), K = input channels x taps, two channels per k-step (lane half h
// supplies channel 2s + h).
//
// A workgroup (4 waves) owns a tile of 8 rows x 32 columns of pixels and MT out-channel tiles of 32; wave w owns the
// pixel rows 2w, 2w + 1 (T = 2) and all MT tiles: MT x T accumulators, and every B value it reads from LDS feeds MT
// MFMAs, every A value T. The input tile with its halo is staged in LDS CK channels at a time, zero-filled outside the
// image and beyond c_in; a channel is a plane of IR rows of PW floats. A ds_read_b32 is served per 32-lane half, so
// the two halves (two different channel planes) never meet on a bank, and within a half the 32 lanes read 32
// consecutive words: stride 1 directly, stride 2 because a row keeps its even columns first and its odd columns
// after them (column c sits at c / 2, or EV + c / 2), which turns the stride-2 walk of a tap into a unit one.
// The weights come fragment-packed in consumption order, [out tile][8 input channels][tap][lane] float4 (element e of
// a lane: row lane & 31, channel 8 c8 + 2 e + (lane >> 5)), behind the folded bias of every GEMM row. A transposed
// convolution is the 1x1 form with c_out * s * s rows (row = (co * s + dy) * s + dx, the weight's own layout) and a
// pixel-shuffle store.
#include "dal3_kernels.h"

namespace {

constexpr int CV_BLOCK = 256, CV_WAVES = 4, CV_T = 2, CV_ROWS = CV_WAVES * CV_T, CV_COLS = 32;

__host__ __device__ constexpr int cv_taps(int kind) { return kind == DAL3_CONV2D_3X3 ? 9 : 1; }
__host__ __device__ constexpr int cv_sub(int kind) { return kind == DAL3_CONV2D_DECONV2 ? 4 : kind == DAL3_CONV2D_DECONV4 ? 16 : 1; }

// (the fold itself: dal3_fold.h. Every index that grows with c_in is 64-bit or a channel number: the RoI head's first
// layer comes here with up to 5 * 65535 inputs)
__global__ __launch_bounds__(CV_BLOCK) void conv2d_pack_kernel(const FoldLayer L, int kind, int n_tiles, int nc8, int64_t total,
                                                               float* out) {
    const int taps = cv_taps(kind), sub = cv_sub(kind), rows = L.c_out * sub;
    for (int64_t i = (int64_t)blockIdx.x * CV_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * CV_BLOCK) {
        float v = 0.f;
        if (i < (int64_t)n_tiles * 32) {
            const int row = (int)i;
            if (row < rows) v = fold_bias(L, row / sub);
        } else {
            const int64_t j = i - (int64_t)n_tiles * 32;
            const int e = (int)(j & 3), lane = (int)((j >> 2) & 63);
            const int64_t t = j >> 8;
            const int tap = (int)(t % taps), c8 = (int)((t / taps) % nc8), ot = (int)(t / ((int64_t)taps * nc8));
            const int row = 32 * ot + (lane & 31), ci = 8 * c8 + 2 * e + (lane >> 5);
            if (row < rows && ci < L.c_in) {
                const int co = row / sub;
                const int64_t at = sub == 1 ? ((int64_t)co * L.c_in + ci) * taps + tap : ((int64_t)ci * L.c_out + co) * sub + row % sub;
                v = fold_weight(L, at, co);
            }
        }
        out[i] = v;
    }
}

struct ConvGeom {
    int c_in, rows, sub, shuffle_s;      // GEMM rows = c_out * sub; shuffle_s: the deconv's s (1 otherwise)
    int relu, nc8, n_groups;             // n_groups: row groups of MT tiles
    int H, W, PH, PW;                    // input size; the GEMM's pixel grid (the output's, or the input's for a deconv)
    int tiles_y, tiles_x;
    int64_t n_work;                      // B * tiles_y * tiles_x * n_groups
    const float* x;
    int64_t xb, xh, xw, xc;
    float* y;                            // channel y_channel_offset of the output
    int64_t yb, yh, yw, yc;
    const float* bias;                   // packed: n_tiles * 32 floats
    const f32x4* frag;                   // [n_tiles][nc8][TAPS][64]
};

// TAPS 9 (3x3, padding 1) or 1; S the convolution's stride; SHUF: pixel-shuffle store; MT out tiles per wave
// (two workgroups a CU: the register budget of two waves per SIMD, which the MT = 2 body would otherwise miss by a few)
template <int TAPS, int S, bool SHUF, int MT>
__global__ __launch_bounds__(CV_BLOCK, 2) void conv2d_kernel(const ConvGeom g) {
    constexpr int KW = TAPS == 9 ? 3 : 1;
    constexpr int IR = (CV_ROWS - 1) * S + KW, IC = (CV_COLS - 1) * S + KW;     // staged rows / columns of a channel
    constexpr int EV = (IC + 1) / 2;                                           // even columns of a row (stride 2)
    constexpr int PW = IC, PS = IR * PW;
    constexpr int CK = S == 1 ? 16 : 8;                                        // channels staged at a time
    __shared__ float tile[CK * PS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int n_chunks = (g.nc8 * 8 + CK - 1) / CK;
    // this lane's B operand of (channel pair e, tap (ky, kx), pixel row j): tile[lds0 + const]
    const int lds0 = h * PS + (wave * CV_T * S) * PW + n;

    for (int64_t work = blockIdx.x; work < g.n_work; work += gridDim.x) {
        const int grp = (int)(work % g.n_groups);
        int64_t rest = work / g.n_groups;
        const int tx = (int)(rest % g.tiles_x);
        rest /= g.tiles_x;
        const int ty = (int)(rest % g.tiles_y), b = (int)(rest / g.tiles_y);
        const int py0 = ty * CV_ROWS, px0 = tx * CV_COLS;
        const int iy0 = py0 * S - (KW == 3 ? 1 : 0), ix0 = px0 * S - (KW == 3 ? 1 : 0);
        const int ot0 = grp * MT;

        f32x16 acc[MT][CV_T];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x16 bias = tile_from_channels(g.bias + 32 * (ot0 + mt), h);
#pragma unroll
            for (int j = 0; j < CV_T; ++j) acc[mt][j] = bias;
        }

        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            __syncthreads();                                   // the previous chunk's (or tile's) reads are done
            const int c0 = chunk * CK;
            for (int i = tid; i < CK * IR * IC; i += CV_BLOCK) {
                const int c = i / (IR * IC), rem = i % (IR * IC), r = rem / IC, col = rem % IC;
                const int iy = iy0 + r, ix = ix0 + col, ci = c0 + c;
                float v = 0.f;
                if (ci < g.c_in && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                    v = g.x[b * g.xb + ci * g.xc + iy * g.xh + ix * g.xw];
                const int at = S == 1 ? col : ((col & 1) ? EV + (col >> 1) : (col >> 1));
                tile[c * PS + r * PW + at] = v;
            }
            __syncthreads();
            // a chunk's CK * TAPS terms are summed from zero and then added to the total: the MFMA's sum is one
            // sequential fma chain, and a chain over all of K = c_in * TAPS (3456 terms for the head's first layer) loses
            // ~sqrt(K / (CK * TAPS)) more than a chain per chunk does
            f32x16 part[MT][CV_T];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < CV_T; ++j) part[mt][j] = f32x16{};
            }
#pragma unroll
            for (int k8 = 0; k8 < CK / 8; ++k8) {
                const int c8 = chunk * (CK / 8) + k8;
                if (c8 < g.nc8) {
#pragma unroll
                    for (int tap = 0; tap < TAPS; ++tap) {
                        const int ky = tap / KW, kx = tap % KW;
                        // column n * S + kx of the row: stride 2 reads the even plane (kx 0, 2) or the odd one (kx 1)
                        const int at = S == 1 ? kx : ((kx & 1) ? EV : (kx >> 1));
                        f32x4 a[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            a[mt] = g.frag[(((int64_t)(ot0 + mt) * g.nc8 + c8) * TAPS + tap) * 64 + lane];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float bv[CV_T];
#pragma unroll
                            for (int j = 0; j < CV_T; ++j)
                                bv[j] = tile[lds0 + (k8 * 8 + 2 * e) * PS + (j * S + ky) * PW + at];
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                                for (int j = 0; j < CV_T; ++j) part[mt][j] = mfma32(a[mt][e], bv[j], part[mt][j]);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < CV_T; ++j) acc[mt][j] += part[mt][j];
            }
        }

        // the store: register r of tile mt is GEMM row 32 (ot0 + mt) + tile_chan(r, h) at pixel (py, px0 + n)
        const int px = px0 + n;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int j = 0; j < CV_T; ++j) {
                const int py = py0 + wave * CV_T + j;
                if (py >= g.PH || px >= g.PW) continue;
                const f32x16 v = g.relu ? relu16(acc[mt][j]) : acc[mt][j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * (ot0 + mt) + tile_chan(r, h);
                    if (row >= g.rows) continue;
                    if (SHUF) {
                        const int s = g.shuffle_s, co = row / g.sub, dy = (row % g.sub) / s, dx = row % s;
                        g.y[b * g.yb + co * g.yc + (int64_t)(py * s + dy) * g.yh + (int64_t)(px * s + dx) * g.yw] = v[r];
                    } else {
                        g.y[b * g.yb + row * g.yc + py * g.yh + px * g.yw] = v[r];
                    }
                }
            }
        }
    }
}

template <int TAPS, int S, bool SHUF>
void launch_mt(const ConvGeom& g, int mt, dim3 grid, hipStream_t s) {
    if (mt == 2) hipLaunchKernelGGL((conv2d_kernel<TAPS, S, SHUF, 2>), grid, dim3(CV_BLOCK), 0, s, g);
    else hipLaunchKernelGGL((conv2d_kernel<TAPS, S, SHUF, 1>), grid, dim3(CV_BLOCK), 0, s, g);
}

}  // namespace

size_t conv2d_pack_floats(int kind, int c_in, int c_out) {
    const int64_t rows = (int64_t)c_out * cv_sub(kind), n_tiles = (rows + 31) / 32, nc8 = (c_in + 7) / 8;
    return (size_t)(n_tiles * 32 + n_tiles * nc8 * cv_taps(kind) * 256);
}

hipError_t launch_conv2d_pack(const FoldLayer& L, int kind, float* out, hipStream_t s) {
    const int64_t rows = (int64_t)L.c_out * cv_sub(kind), total = (int64_t)conv2d_pack_floats(kind, L.c_in, L.c_out);
    int64_t blocks = (total + CV_BLOCK - 1) / CV_BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(conv2d_pack_kernel, dim3((unsigned)blocks), dim3(CV_BLOCK), 0, s, L, kind, (int)((rows + 31) / 32),
                       (L.c_in + 7) / 8, total, out);
    return hipGetLastError();
}

hipError_t launch_conv2d(const dal3_conv2d_args* args, hipStream_t s) {
    const dal3_conv2d_args& a = *args;
    if (a.B <= 0 || a.H <= 0 || a.W <= 0) return hipSuccess;
    ConvGeom g = {};
    const bool deconv = a.kind == DAL3_CONV2D_DECONV2 || a.kind == DAL3_CONV2D_DECONV4;
    g.c_in = a.c_in;
    g.sub = cv_sub(a.kind);
    g.shuffle_s = deconv ? a.stride : 1;
    g.rows = a.c_out * g.sub;
    g.relu = a.relu;
    g.nc8 = (a.c_in + 7) / 8;
    const int n_tiles = (g.rows + 31) / 32, mt = n_tiles % 2 == 0 ? 2 : 1;
    g.n_groups = n_tiles / mt;
    g.H = (int)a.H;
    g.W = (int)a.W;
    const int cs = a.kind == DAL3_CONV2D_3X3 ? a.stride : 1;
    g.PH = (g.H - 1) / cs + 1;
    g.PW = (g.W - 1) / cs + 1;
    g.tiles_y = (g.PH + CV_ROWS - 1) / CV_ROWS;
    g.tiles_x = (g.PW + CV_COLS - 1) / CV_COLS;
    g.n_work = a.B * g.tiles_y * g.tiles_x * g.n_groups;
    g.x = a.x.data;
    g.xb = a.x.stride_b, g.xh = a.x.stride_h, g.xw = a.x.stride_w, g.xc = a.x.stride_c;
    g.y = const_cast<float*>(a.y.data) + (int64_t)a.y_channel_offset * a.y.stride_c;
    g.yb = a.y.stride_b, g.yh = a.y.stride_h, g.yw = a.y.stride_w, g.yc = a.y.stride_c;
    g.bias = a.packed;
    g.frag = reinterpret_cast<const f32x4*>(a.packed + (int64_t)n_tiles * 32);
    int64_t blocks = g.n_work;
    if (a.max_workgroups > 0 && blocks > a.max_workgroups) blocks = a.max_workgroups;
    if (blocks > 0x7fffffff) blocks = 0x7fffffff;
    const dim3 grid((unsigned)blocks);
    if (a.kind == DAL3_CONV2D_3X3 && a.stride == 1) launch_mt<9, 1, false>(g, mt, grid, s);
    else if (a.kind == DAL3_CONV2D_3X3) launch_mt<9, 2, false>(g, mt, grid, s);
    else if (a.kind == DAL3_CONV2D_1X1) launch_mt<1, 1, false>(g, mt, grid, s);
    else launch_mt<1, 1, true>(g, mt, grid, s);
    return hipGetLastError();
}
