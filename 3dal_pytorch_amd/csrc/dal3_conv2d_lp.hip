// dal3_conv2d_lp.hip — the detector's dense stage on 16-bit MFMA operands (dal3_conv2d_lp_pack / dal3_conv2d_lp of
// include/dal3.h): the four forms of dal3_conv2d.hip (3x3 of stride 1 and 2, 1x1, the k = s transposed forms as 1x1 with
// a pixel-shuffle store) as ONE implicit-GEMM body on v_mfma_f32_32x32x16_{f16,bf16}, in the fp32 body's orientation:
// output channels (GEMM rows) on the MFMA rows, 32 output pixels of one image row on its columns (= lanes), K = input
// channels x taps, 16 channels per k-step (lane half h supplies channels 8h .. 8h + 7 of its pixel).
//
// The arithmetic (the contract of include/dal3.h): the folded weight W' (dal3_fold.h: float64 fold, one rounding to float32)
// is rounded once more, to the 16-bit type, by the packer; every input activation is rounded to the 16-bit type as it is
// staged; both roundings are to nearest even. Products are summed in the MFMA's fp32 accumulator, which starts at the fp32
// folded bias b'; ReLU and the store are fp32. The maps stay float32 NCHW behind dal3_map strides.
//
// A workgroup (4 waves) owns 8 rows x 32 columns of pixels and MT out-channel tiles of 32; wave w owns the pixel rows 2w,
// 2w + 1 (T = 2) and all MT tiles, as in the fp32 body. The input tile with its halo is staged CK channels at a time
// channel-innermost: a 16-byte unit holds 8 channels of one pixel, a plane holds the units of one block of 8 channels
// ([plane][row][column]), zero-filled outside the image and beyond c_in. The B operand of a tap is then one ds_read_b128
// per lane at unit lane stride (16 lanes x 16 B cover the 64 banks once; the two lane halves read different planes in
// different LDS cycles). Stride 2 keeps the fp32 body's split of a row into its even columns and then its odd ones, so
// that the stride-2 walk of a tap is a unit one.
//
// Weights: [fp32 bias of every GEMM row | fragments by out tile], a fragment being the A operand of one (out tile, 16
// input channels, tap): 64 lanes x 8 values, lane (m, h) holding W'[row m][channel 16 k + 8h + j]. At 32 cycles per MFMA a
// wave with MT = T = 2 needs 2 KiB of A every 128 cycles; four waves reading the same fragments straight from global
// memory would ask the L1 for four times that. So a chunk's fragments (MT x CK / 16 x taps of 1 KiB) are STAGED PLAINLY in
// LDS beside the input chunk, once per workgroup, and every wave reads them back with ds_read_b128: per MFMA one LDS read
// (MT A reads and T B reads feed MT x T MFMAs), half of what the LDS array serves per 32-cycle gap with four waves a CU
// side (4 cycles per wave-instruction, 256 B/clk). LdsRing (dal3_lp.h) was not taken: its LDS-DMA stream wants ONE
// consumption order for the whole kernel, and here the order is per (work item, chunk) with the input staging's ordinary
// global loads in the same loop, which the ring's counted vmcnt waits do not tolerate. The staging is not overlapped with
// the MFMAs of the same workgroup; two workgroups a CU overlap each other.
//
// Chunked partial sums, the fp32 body's rule: a chunk's CK x taps terms are summed from zero and then added to the total.
#include "dal3_kernels.h"
#include "dal3_lp.h"

namespace {

constexpr int CL_BLOCK = 256, CL_WAVES = 4, CL_T = 2, CL_ROWS = CL_WAVES * CL_T, CL_COLS = 32;

__host__ __device__ constexpr int cl_taps(int kind) { return kind == DAL3_CONV2D_3X3 ? 9 : 1; }
__host__ __device__ constexpr int cl_sub(int kind) { return kind == DAL3_CONV2D_DECONV2 ? 4 : kind == DAL3_CONV2D_DECONV4 ? 16 : 1; }

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// one float -> the 16-bit type, round to nearest even (the conversions' default), as its bit pattern
template <class DT>
__device__ __forceinline__ uint16_t round16(float v) {
    return __builtin_bit_cast(uint16_t, (typename DT::elem)v);
}

// the blob: n_tiles * 32 fp32 biases, then [out tile][nk16][tap][lane][8] 16-bit values
template <class DT>
__global__ __launch_bounds__(CL_BLOCK) void conv2d_lp_pack_kernel(const FoldLayer L, int kind, int n_tiles, int nk16, int64_t n_values,
                                                                  float* bias, uint16_t* frag) {
    const int taps = cl_taps(kind), sub = cl_sub(kind), rows = L.c_out * sub;
    for (int64_t i = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x; i < n_values + n_tiles * 32; i += (int64_t)gridDim.x * CL_BLOCK) {
        if (i < n_tiles * 32) {
            const int row = (int)i;
            bias[row] = row < rows ? fold_bias(L, row / sub) : 0.f;
            continue;
        }
        const int64_t j = i - n_tiles * 32;
        const int e = (int)(j & 7), lane = (int)((j >> 3) & 63);
        const int64_t t = j >> 9;
        const int tap = (int)(t % taps), k16 = (int)((t / taps) % nk16), ot = (int)(t / ((int64_t)taps * nk16));
        const int row = 32 * ot + (lane & 31), ci = 16 * k16 + 8 * (lane >> 5) + e;
        float v = 0.f;
        if (row < rows && ci < L.c_in) {
            const int co = row / sub;
            const int64_t at = sub == 1 ? ((int64_t)co * L.c_in + ci) * taps + tap : ((int64_t)ci * L.c_out + co) * sub + row % sub;
            v = fold_weight(L, at, co);
            // W' is a float32 VALUE before it is rounded to 16 bits (two roundings, the contract's): left to itself the
            // compiler converts the float64 product straight to 16 bits, which differs wherever the float32 lands on a tie
            asm volatile("" : "+v"(v));
        }
        frag[j] = round16<DT>(v);
    }
}

struct ConvLpGeom {
    int c_in, rows, sub, shuffle_s;      // GEMM rows = c_out * sub; shuffle_s: the deconv's s (1 otherwise)
    int shuffle_log2;                    // log2 of shuffle_s
    int relu, nk16, n_groups;            // nk16: k-steps of 16 channels; n_groups: row groups of MT tiles
    int H, W, PH, PW;                    // input size; the GEMM's pixel grid (the output's, or the input's for a deconv)
    int tiles_y, tiles_x;
    int64_t n_work;                      // B * tiles_y * tiles_x * n_groups
    const float* x;
    int64_t xb, xh, xw, xc;
    float* y;                            // channel y_channel_offset of the output
    int64_t yb, yh, yw, yc;
    const float* bias;                   // packed: n_tiles * 32 floats
    const u32x4_t* frag;                 // [n_tiles][nk16][TAPS][64]
};

// TAPS 9 (3x3, padding 1) or 1; S the convolution's stride; SHUF: pixel-shuffle store; MT out tiles per wave
template <class DT, int TAPS, int S, bool SHUF, int MT>
__global__ __launch_bounds__(CL_BLOCK, 2) void conv2d_lp_kernel(const ConvLpGeom g) {
    constexpr int KW = TAPS == 9 ? 3 : 1;
    constexpr int IR = (CL_ROWS - 1) * S + KW, IC = (CL_COLS - 1) * S + KW;     // staged rows / columns of a plane
    constexpr int EV = (IC + 1) / 2;                                           // even columns of a row (stride 2)
    constexpr int PW = IC, PS = IR * PW;                                       // units per row / per plane
    constexpr int CK = S == 1 ? 32 : 16, KS = CK / 16, NP = CK / 8;            // channels, k-steps and planes of a chunk
    __shared__ u32x4_t tile[NP * PS];
    __shared__ u32x4_t wfrag[MT * KS * TAPS * 64];
    typedef typename DT::v8 v8;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int n_chunks = (g.nk16 + KS - 1) / KS;
    // this lane's B operand of (k-step ks, tap (ky, kx), pixel row j): tile[lds0 + const]
    const int lds0 = h * PS + (wave * CL_T * S) * PW + n;

    for (int64_t work = blockIdx.x; work < g.n_work; work += gridDim.x) {
        const int grp = (int)(work % g.n_groups);
        int64_t rest = work / g.n_groups;
        const int tx = (int)(rest % g.tiles_x);
        rest /= g.tiles_x;
        const int ty = (int)(rest % g.tiles_y), b = (int)(rest / g.tiles_y);
        const int py0 = ty * CL_ROWS, px0 = tx * CL_COLS;
        const int iy0 = py0 * S - (KW == 3 ? 1 : 0), ix0 = px0 * S - (KW == 3 ? 1 : 0);
        const int ot0 = grp * MT;

        f32x16 acc[MT][CL_T];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x16 bias = tile_from_channels(g.bias + 32 * (ot0 + mt), h);
#pragma unroll
            for (int j = 0; j < CL_T; ++j) acc[mt][j] = bias;
        }

        for (int chunk = 0; chunk < n_chunks; ++chunk) {
            __syncthreads();                                   // the previous chunk's (or tile's) reads are done
            const int c0 = chunk * CK;
            // the input: one unit (8 channels of a pixel) per thread and turn, consecutive lanes on consecutive columns
            for (int i = tid; i < NP * IR * IC; i += CL_BLOCK) {
                const int p = i / (IR * IC), rem = i % (IR * IC), r = rem / IC, col = rem % IC;
                const int iy = iy0 + r, ix = ix0 + col, ci0 = c0 + 8 * p;
                u32x4_t unit = {0u, 0u, 0u, 0u};
                if (ci0 < g.c_in && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) {
                    const float* src = g.x + b * g.xb + iy * g.xh + ix * g.xw;
                    float v[8];
                    // (eight independent loads, the channel clamped and the value dropped past c_in: a load under its own
                    // condition waits for the one before it)
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = src[(ci0 + j < g.c_in ? ci0 + j : g.c_in - 1) * g.xc];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = ci0 + j < g.c_in ? v[j] : 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        unit[j] = (uint32_t)round16<DT>(v[2 * j]) | ((uint32_t)round16<DT>(v[2 * j + 1]) << 16);
                }
                const int at = S == 1 ? col : ((col & 1) ? EV + (col >> 1) : (col >> 1));
                tile[p * PS + r * PW + at] = unit;
            }
            // the chunk's fragments of the MT out tiles: [mt][ks][tap][lane]
            for (int i = tid; i < MT * KS * TAPS * 64; i += CL_BLOCK) {
                const int f = i >> 6, tap = f % TAPS, ks = (f / TAPS) % KS, mt = f / (TAPS * KS), k16 = chunk * KS + ks;
                if (k16 < g.nk16) wfrag[i] = g.frag[(((int64_t)(ot0 + mt) * g.nk16 + k16) * TAPS + tap) * 64 + (i & 63)];
            }
            __syncthreads();
            f32x16 part[MT][CL_T];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < CL_T; ++j) part[mt][j] = f32x16{};
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (chunk * KS + ks < g.nk16) {
#pragma unroll
                    for (int tap = 0; tap < TAPS; ++tap) {
                        const int ky = tap / KW, kx = tap % KW;
                        // column n * S + kx of the row: stride 2 reads the even part (kx 0, 2) or the odd one (kx 1)
                        const int at = S == 1 ? kx : ((kx & 1) ? EV : (kx >> 1));
                        v8 a[MT], bv[CL_T];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) a[mt] = __builtin_bit_cast(v8, wfrag[((mt * KS + ks) * TAPS + tap) * 64 + lane]);
#pragma unroll
                        for (int j = 0; j < CL_T; ++j) bv[j] = __builtin_bit_cast(v8, tile[lds0 + 2 * ks * PS + (j * S + ky) * PW + at]);
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                            for (int j = 0; j < CL_T; ++j) part[mt][j] = DT::mfma(a[mt], bv[j], part[mt][j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int j = 0; j < CL_T; ++j) acc[mt][j] += part[mt][j];
            }
        }

        // the store: register r of tile mt is GEMM row 32 (ot0 + mt) + tile_chan(r, h) at pixel (py, px0 + n)
        const int px = px0 + n;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int j = 0; j < CL_T; ++j) {
                const int py = py0 + wave * CL_T + j;
                if (py >= g.PH || px >= g.PW) continue;
                const f32x16 v = g.relu ? relu16(acc[mt][j]) : acc[mt][j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * (ot0 + mt) + tile_chan(r, h);
                    if (row >= g.rows) continue;
                    if (SHUF) {
                        // s is 2 or 4 and sub = s * s: shifts and masks, not the divisions by a runtime value
                        const int s = g.shuffle_s, ls = g.shuffle_log2, co = row >> (2 * ls), dy = (row >> ls) & (s - 1), dx = row & (s - 1);
                        g.y[b * g.yb + co * g.yc + (int64_t)(py * s + dy) * g.yh + (int64_t)(px * s + dx) * g.yw] = v[r];
                    } else {
                        g.y[b * g.yb + row * g.yc + py * g.yh + px * g.yw] = v[r];
                    }
                }
            }
        }
    }
}

template <class DT, int TAPS, int S, bool SHUF>
void launch_mt(const ConvLpGeom& g, int mt, dim3 grid, hipStream_t s) {
    if (mt == 2) hipLaunchKernelGGL((conv2d_lp_kernel<DT, TAPS, S, SHUF, 2>), grid, dim3(CL_BLOCK), 0, s, g);
    else hipLaunchKernelGGL((conv2d_lp_kernel<DT, TAPS, S, SHUF, 1>), grid, dim3(CL_BLOCK), 0, s, g);
}

template <class DT>
void launch_form(const ConvLpGeom& g, int kind, int stride, int mt, dim3 grid, hipStream_t s) {
    if (kind == DAL3_CONV2D_3X3 && stride == 1) launch_mt<DT, 9, 1, false>(g, mt, grid, s);
    else if (kind == DAL3_CONV2D_3X3) launch_mt<DT, 9, 2, false>(g, mt, grid, s);
    else if (kind == DAL3_CONV2D_1X1) launch_mt<DT, 1, 1, false>(g, mt, grid, s);
    else launch_mt<DT, 1, 1, true>(g, mt, grid, s);
}

}  // namespace

size_t conv2d_lp_pack_bytes(int kind, int c_in, int c_out) {
    const int64_t rows = (int64_t)c_out * cl_sub(kind), n_tiles = (rows + 31) / 32, nk16 = (c_in + 15) / 16;
    return (size_t)(n_tiles * 32 * 4 + n_tiles * nk16 * cl_taps(kind) * 1024);
}

hipError_t launch_conv2d_lp_pack(const FoldLayer& L, int kind, int dtype, void* out, hipStream_t s) {
    const int64_t rows = (int64_t)L.c_out * cl_sub(kind), n_tiles = (rows + 31) / 32, nk16 = (L.c_in + 15) / 16;
    const int64_t n_values = n_tiles * nk16 * cl_taps(kind) * 512, total = n_values + n_tiles * 32;
    int64_t blocks = (total + CL_BLOCK - 1) / CL_BLOCK;
    if (blocks > 4096) blocks = 4096;
    float* bias = static_cast<float*>(out);
    uint16_t* frag = reinterpret_cast<uint16_t*>(bias + n_tiles * 32);
    if (dtype == DAL3_F16)
        hipLaunchKernelGGL(conv2d_lp_pack_kernel<FP16>, dim3((unsigned)blocks), dim3(CL_BLOCK), 0, s, L, kind, (int)n_tiles, (int)nk16,
                           n_values, bias, frag);
    else
        hipLaunchKernelGGL(conv2d_lp_pack_kernel<BF16>, dim3((unsigned)blocks), dim3(CL_BLOCK), 0, s, L, kind, (int)n_tiles, (int)nk16,
                           n_values, bias, frag);
    return hipGetLastError();
}

hipError_t launch_conv2d_lp(const dal3_conv2d_lp_args* args, hipStream_t s) {
    const dal3_conv2d_lp_args& a = *args;
    if (a.B <= 0 || a.H <= 0 || a.W <= 0) return hipSuccess;
    ConvLpGeom g = {};
    const bool deconv = a.kind == DAL3_CONV2D_DECONV2 || a.kind == DAL3_CONV2D_DECONV4;
    g.c_in = a.c_in;
    g.sub = cl_sub(a.kind);
    g.shuffle_s = deconv ? a.stride : 1;
    g.shuffle_log2 = g.shuffle_s == 4 ? 2 : g.shuffle_s == 2 ? 1 : 0;
    g.rows = a.c_out * g.sub;
    g.relu = a.relu;
    g.nk16 = (a.c_in + 15) / 16;
    const int n_tiles = (g.rows + 31) / 32, mt = n_tiles % 2 == 0 ? 2 : 1;
    g.n_groups = n_tiles / mt;
    g.H = (int)a.H;
    g.W = (int)a.W;
    const int cs = a.kind == DAL3_CONV2D_3X3 ? a.stride : 1;
    g.PH = (g.H - 1) / cs + 1;
    g.PW = (g.W - 1) / cs + 1;
    g.tiles_y = (g.PH + CL_ROWS - 1) / CL_ROWS;
    g.tiles_x = (g.PW + CL_COLS - 1) / CL_COLS;
    g.n_work = a.B * g.tiles_y * g.tiles_x * g.n_groups;
    g.x = a.x.data;
    g.xb = a.x.stride_b, g.xh = a.x.stride_h, g.xw = a.x.stride_w, g.xc = a.x.stride_c;
    g.y = const_cast<float*>(a.y.data) + (int64_t)a.y_channel_offset * a.y.stride_c;
    g.yb = a.y.stride_b, g.yh = a.y.stride_h, g.yw = a.y.stride_w, g.yc = a.y.stride_c;
    g.bias = static_cast<const float*>(a.packed);
    g.frag = reinterpret_cast<const u32x4_t*>(g.bias + (int64_t)n_tiles * 32);
    int64_t blocks = g.n_work;
    if (a.max_workgroups > 0 && blocks > a.max_workgroups) blocks = a.max_workgroups;
    if (blocks > 0x7fffffff) blocks = 0x7fffffff;
    const dim3 grid((unsigned)blocks);
    if (a.dtype == DAL3_F16) launch_form<FP16>(g, a.kind, a.stride, mt, grid, s);
    else launch_form<BF16>(g, a.kind, a.stride, mt, grid, s);
    return hipGetLastError();
}
