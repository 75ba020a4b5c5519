// dal3_pillars_train.hip — the PointPillars reader's training step (dal3_pillar_train_forward / dal3_pillar_train_backward,
// include/dal3.h): PFNLayer of det3d/models/readers/pillar_encoder.py:40-55 in train mode, forward and backward.
//
// Every pass is dal3_pillars.hip's feature kernel again: one wave per pillar, channels on the fp32 MFMA's rows and the
// pillar's rows on its columns, the layers chained through the accumulators. A pass recomputes the forward from the
// voxels; nothing of size P * max_points * channels is ever stored. Between two passes lies a sum over all pillars
// (BatchNorm's statistics, then its backward's two sums), so the step is a chain of passes with a small kernel between:
//   forward    F1  sum z1, sum z1^2            -> mean1, istd1, the running statistics
//              F2  the same of layer 2 (runs layer 1 with its batch statistics; two-layer nets only)
//              F3  the outputs
//   backward   B1  dbeta, dgamma of the last layer (the argmax rows are found again, not stored)
//              B2  dz2 -> dW2, dx2 -> da1 -> dbeta1, dgamma1 (two-layer nets only)
//              B3  dz1 -> dW1
// dW contracts over the pillar's rows, which the accumulators hold on the lanes: dz and the layer's input go through the
// wave's own LDS rows ([channel][row], an odd stride) and come back as A and B operands with the rows on k.
//
// The sums. A wave owns a SLICE of DAL3_PILLAR_TRAIN_SLICE consecutive pillars, walks it in order and adds what a pillar
// contributes to float64 registers; the slice's partial is stored and the pt_finish_* kernels add the partials in
// ascending slice order, in float64. Which wave of which workgroup takes a slice changes nothing of this, so the bits
// are those of the input alone for every max_workgroups and every run; there is no floating-point atomic. The MFMA
// columns beyond max_points repeat the pillar's last row (max-invariant, not sum-invariant): every sum masks them.
//
// Ties of the max. The cotangent of a max goes to the lowest row that attains it. Rows that tie exactly are either at
// y = 0, where the ReLU gate stops the cotangent whichever row is picked, or rows with identical inputs (padding rows,
// duplicated points): those have the same z, x-hat and layer input, so dbeta, dgamma and dW get the same terms from
// whichever of them is picked. The choice therefore never shows in a parameter gradient.
#include "dal3_block.h"
#include "dal3_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int PT_S = DAL3_PILLAR_TRAIN_SLICE;
constexpr int PT_KS = 7;                        // k-steps of layer 1: C + 5 <= 13 inputs, two a step
constexpr int PT_K = 4096 + 64;                 // doubles of a slice's partial: the widest pass's (dW2, dbeta1, dgamma1)
constexpr int PT_SAVED_LAYER = 256;             // saved: per layer mean | istd | scale = gamma istd | shift = beta - mean scale
constexpr int PT_BCO_LAYER = 128;               // backward coefficients: per layer dbeta / n | dgamma / n
enum { PT_F1, PT_F2, PT_F3, PT_B1, PT_B2, PT_B3 };

__host__ __device__ constexpr int pt_waves(int NT) { return NT == 1 ? 4 : 2; }
__host__ __device__ constexpr int pt_ld(int NT) { return 32 * NT + 1; }
// a wave's LDS floats: dz [64][LD] | the layer's input [32][LD] | the pillar's layer-1 maximum [32]
__host__ __device__ constexpr int pt_wave_floats(int NT) { return 96 * pt_ld(NT) + 32; }

struct PtArgs {
    int64_t P;
    const int64_t* n_pillars;
    const float* voxels;
    const int32_t* num_points;
    const int32_t* coords;
    int C, T;
    float vx, vy, xo, yo;
    const float *W1, *W2;
    const float* saved;
    const float* bco;
    float* features;
    float* canvas;
    int64_t canvas_B, ny, nx;
    const float* grad;
    int64_t gs[4];
    double* part;
};

__device__ __forceinline__ int64_t pt_live(int64_t P, const int64_t* n_pillars) {
    if (!n_pillars) return P;
    const int64_t live = *n_pillars;
    return live < 0 ? 0 : live < P ? live : P;
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
    return t;
}

__device__ __forceinline__ f32x16 pt_max_over_columns(f32x16 a) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = fmaxf(a[r], __shfl_xor(a[r], off, 64));
    }
    return a;
}

// the sum over the 32 lanes of a half, in a fixed order
__device__ __forceinline__ double pt_sum_columns(double v) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// y = relu(z * scale + shift), one fused multiply-add in every pass
template <int NT, int MT>
__device__ __forceinline__ void pt_act(const f32x16 (&z)[NT][MT], const f32x16 (&sc)[MT], const f32x16 (&sh)[MT],
                                       f32x16 (&y)[NT][MT], f32x16 (&top)[MT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) y[j][mt][r] = fmaxf(__builtin_fmaf(z[j][mt][r], sc[mt][r], sh[mt][r]), 0.f);
        }
        f32x16 m = y[0][mt];
#pragma unroll
        for (int j = 1; j < NT; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) m[r] = fmaxf(m[r], y[j][mt][r]);
        }
        top[mt] = pt_max_over_columns(m);
    }
}

// first[j][mt][r]: this lane's column is the lowest real row of the pillar at which the channel attains its maximum
template <int NT, int MT>
__device__ __forceinline__ void pt_first_max(const f32x16 (&y)[NT][MT], const f32x16 (&top)[MT], int n, int T,
                                             bool (&first)[NT][MT][16]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int mine = 255;
#pragma unroll
            for (int j = NT - 1; j >= 0; --j) mine = (32 * j + n < T && y[j][mt][r] == top[mt][r]) ? 32 * j + n : mine;
            int low = mine;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                const int o = __shfl_xor(low, off, 64);
                low = o < low ? o : low;
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) first[j][mt][r] = low < 255 && 32 * j + n == low;
        }
    }
}

// two per-channel sums of a slice (tile layout: register r of half h is channel 32 mt + tile_chan(r, h)) -> the partial
template <int MT>
__device__ __forceinline__ void pt_store_pair(const double (&qa)[2][16], const double (&qb)[2][16], double* part, int off_a,
                                              int off_b, int n, int h) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double sa = pt_sum_columns(qa[mt][r]), sb = pt_sum_columns(qb[mt][r]);
            if (n == 0) {
                part[off_a + 32 * mt + tile_chan(r, h)] = sa;
                part[off_b + 32 * mt + tile_chan(r, h)] = sb;
            }
        }
    }
}

template <int MT>
__device__ __forceinline__ void pt_tiles(const float* v, int h, f32x16 (&t)[MT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) t[mt] = tile_from_channels(v + 32 * mt, h);
}

// dz = scale * (da - dbeta / n - xhat * dgamma / n) on the real rows, 0 on the tile's padding columns
template <int NT, int MT>
__device__ __forceinline__ void pt_dz(const f32x16 (&da)[NT][MT], const f32x16 (&z)[NT][MT], const float* saved, const float* bco,
                                      int n, int h, int T, f32x16 (&dz)[NT][MT]) {
    f32x16 mean[MT], istd[MT], sc[MT], mb[MT], mg[MT];
    pt_tiles<MT>(saved, h, mean);
    pt_tiles<MT>(saved + 64, h, istd);
    pt_tiles<MT>(saved + 128, h, sc);
    pt_tiles<MT>(bco, h, mb);
    pt_tiles<MT>(bco + 64, h, mg);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const bool real = 32 * j + n < T;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float xh = (z[j][mt][r] - mean[mt][r]) * istd[mt][r];
                const float v = sc[mt][r] * ((da[j][mt][r] - mb[mt][r]) - xh * mg[mt][r]);
                dz[j][mt][r] = real ? v : 0.f;
            }
        }
    }
}

// qa += da, qb += da * xhat over the real rows
template <int NT, int MT>
__device__ __forceinline__ void pt_add_bn_sums(const f32x16 (&da)[NT][MT], const f32x16 (&z)[NT][MT], const float* saved, int n,
                                               int h, int T, double (&qa)[2][16], double (&qb)[2][16]) {
    f32x16 mean[MT], istd[MT];
    pt_tiles<MT>(saved, h, mean);
    pt_tiles<MT>(saved + 64, h, istd);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        if (32 * j + n >= T) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float xh = (z[j][mt][r] - mean[mt][r]) * istd[mt][r];
                qa[mt][r] += (double)da[j][mt][r];
                qb[mt][r] += (double)da[j][mt][r] * (double)xh;
            }
        }
    }
}

// the accumulator tiles of NT column tiles -> the wave's LDS rows [channel][column]
template <int NT, int MT>
__device__ __forceinline__ void pt_to_lds(const f32x16 (&t)[NT][MT], float* rows, int n, int h) {
    constexpr int LD = pt_ld(NT);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) rows[(32 * mt + tile_chan(r, h)) * LD + 32 * j + n] = t[j][mt][r];
        }
    }
}

__device__ __forceinline__ void pt_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// TWO: units [32, 64], else [64]; NT: column tiles (max_points > 32: 2). Workgroup: pt_waves(NT) waves, a slice each.
template <int MODE, bool TWO, int NT>
__global__ __launch_bounds__(64 * pt_waves(NT)) void pt_pass_kernel(const PtArgs a) {
    constexpr int WAVES = pt_waves(NT), LD = pt_ld(NT), MT1 = TWO ? 1 : 2;
    constexpr bool BWD = MODE >= PT_B1;
    extern __shared__ __attribute__((aligned(16))) float pt_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
    float* dzs = pt_smem + wave * pt_wave_floats(NT);       // [64][LD]
    float* xs = dzs + 64 * LD;                              // [32][LD]
    float* tops = xs + 32 * LD;                             // [32]
    const int64_t P = pt_live(a.P, a.n_pillars);
    const int c_in = a.C + 5, T = a.T;

    // the A operands of the forward stay in registers over the wave's pillars
    float a1[MT1][PT_KS], a2a[TWO ? 2 : 1][16], a2b[TWO ? 2 : 1][16];
#pragma unroll
    for (int mt = 0; mt < MT1; ++mt) {
#pragma unroll
        for (int s = 0; s < PT_KS; ++s) {
            const int k = 2 * s + h;
            a1[mt][s] = k < c_in ? a.W1[(32 * mt + n) * c_in + k] : 0.f;
        }
    }
    if constexpr (TWO && MODE != PT_F1) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                a2a[mt][s] = a.W2[(32 * mt + n) * 64 + tile_chan(s, h)];
                a2b[mt][s] = a.W2[(32 * mt + n) * 64 + 32 + tile_chan(s, h)];
            }
        }
    }
    f32x16 sc1[MT1], sh1[MT1], sc2[2], sh2[2];
    if constexpr (MODE != PT_F1) {
        pt_tiles<MT1>(a.saved + 128, h, sc1);
        pt_tiles<MT1>(a.saved + 192, h, sh1);
    }
    if constexpr (TWO && MODE != PT_F1 && MODE != PT_F2) {
        pt_tiles<2>(a.saved + PT_SAVED_LAYER + 128, h, sc2);
        pt_tiles<2>(a.saved + PT_SAVED_LAYER + 192, h, sh2);
    }

    for (int64_t slice = (int64_t)blockIdx.x * WAVES + wave; slice * PT_S < P; slice += (int64_t)gridDim.x * WAVES) {
        double* part = a.part + slice * PT_K;
        double qa[2][16], qb[2][16];                        // two per-channel sums
        double dw[TWO ? 2 : 1][2][16];                      // B2: dW2's four tiles; B3: dW1's MT1 tiles in dw[0]
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                qa[i][r] = qb[i][r] = 0.0;
#pragma unroll
                for (int m = 0; m < (TWO ? 2 : 1); ++m) dw[m][i][r] = 0.0;
            }
        }
        const int64_t p_end = (slice + 1) * PT_S < P ? (slice + 1) * PT_S : P;
        for (int64_t p = slice * PT_S; p < p_end; ++p) {
            const float* vox = a.voxels + p * T * a.C;
            const int32_t* co = a.coords + 4 * p;
            const int32_t np = a.num_points[p];
            float sx = 0.f, sy = 0.f, sz = 0.f;
            for (int r = 0; r < T; ++r) {
                sx += vox[r * a.C];
                sy += vox[r * a.C + 1];
                sz += vox[r * a.C + 2];
            }
            const float cnt = (float)np;
            const float mx = __fdiv_rn(sx, cnt), my = __fdiv_rn(sy, cnt), mz = __fdiv_rn(sz, cnt);
            const float cx = (float)co[3] * a.vx + a.xo, cy = (float)co[2] * a.vy + a.yo;
            // ---- layer 1: z1 = W1 x
            float in[NT][PT_KS];
            f32x16 z1[NT][MT1];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                int r = 32 * j + n;
                r = r < T ? r : T - 1;                      // columns beyond the pillar repeat its last row
                const float* row = vox + r * a.C;
                float f[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) f[c] = c < a.C ? row[c] : 0.f;
                const float dec[5] = {f[0] - mx, f[1] - my, f[2] - mz, f[0] - cx, f[1] - cy};
                const float mask = r < np ? 1.f : 0.f;
#pragma unroll
                for (int s = 0; s < PT_KS; ++s) {
                    const int k = 2 * s + h;
                    float v = 0.f;
#pragma unroll
                    for (int d = 0; d < 5; ++d) v = k - a.C == d ? dec[d] : v;
#pragma unroll
                    for (int c = 0; c < 8; ++c) v = k == c && c < a.C ? f[c] : v;
                    in[j][s] = r < np ? v * mask : 0.f;     // (a padding row is exactly 0 whatever its voxel holds)
                }
#pragma unroll
                for (int mt = 0; mt < MT1; ++mt) {
                    f32x16 acc = zero16();
#pragma unroll
                    for (int s = 0; s < PT_KS; ++s) acc = mfma32(a1[mt][s], in[j][s], acc);
                    z1[j][mt] = acc;
                }
            }
            if constexpr (MODE == PT_F1) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    if (32 * j + n >= T) continue;
#pragma unroll
                    for (int mt = 0; mt < MT1; ++mt) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const double z = (double)z1[j][mt][r];
                            qa[mt][r] += z;
                            qb[mt][r] += z * z;
                        }
                    }
                }
                continue;
            }
            f32x16 y1[NT][MT1], top1[MT1];
            pt_act<NT, MT1>(z1, sc1, sh1, y1, top1);
            // ---- the last layer's z, y and maximum
            f32x16 zl[NT][2], yl[NT][2], topl[2];
            if constexpr (TWO) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    f32x16 term = zero16();
#pragma unroll
                    for (int s = 0; s < 16; ++s) term = mfma32(a2b[mt][s], top1[0][s], term);
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        f32x16 acc = term;
#pragma unroll
                        for (int s = 0; s < 16; ++s) acc = mfma32(a2a[mt][s], y1[j][0][s], acc);
                        zl[j][mt] = acc;
                    }
                }
                if constexpr (MODE == PT_F2) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        if (32 * j + n >= T) continue;
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const double z = (double)zl[j][mt][r];
                                qa[mt][r] += z;
                                qb[mt][r] += z * z;
                            }
                        }
                    }
                    continue;
                }
                pt_act<NT, 2>(zl, sc2, sh2, yl, topl);
            } else {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    topl[mt] = top1[mt % MT1];
#pragma unroll
                    for (int j = 0; j < NT; ++j) zl[j][mt] = z1[j][mt % MT1], yl[j][mt] = y1[j][mt % MT1];
                }
            }
            const int64_t cb = co[0], cyi = co[2], cxi = co[3];
            const bool on_canvas = cb >= 0 && cb < a.canvas_B && cyi >= 0 && cyi < a.ny && cxi >= 0 && cxi < a.nx;
            if constexpr (MODE == PT_F3) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    float v = topl[mt][0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) v = n == r ? topl[mt][r] : v;
                    if (n >= 16) continue;
                    const int ch = 32 * mt + tile_chan(n, h);
                    if (a.canvas) {
                        if (on_canvas) a.canvas[((cb * 64 + ch) * a.ny + cyi) * a.nx + cxi] = v;
                    } else {
                        a.features[p * 64 + ch] = v;
                    }
                }
                continue;
            }
            if constexpr (BWD) {
            // ---- the cotangent of the last layer's maximum, at its first row, behind the ReLU's gate
            const float* sv_l = a.saved + (TWO ? PT_SAVED_LAYER : 0);
            const float* bco_l = a.bco + (TWO ? PT_BCO_LAYER : 0);
            f32x16 dal[NT][2];
            {
                bool first[NT][2][16];
                pt_first_max<NT, 2>(yl, topl, n, T, first);
                const bool have = a.canvas ? on_canvas : true;
                const int64_t base = a.canvas ? cb * a.gs[0] + cyi * a.gs[2] + cxi * a.gs[3] : p * a.gs[0];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ch = 32 * mt + tile_chan(r, h);
                        const float g = have ? a.grad[base + ch * a.gs[1]] : 0.f;
#pragma unroll
                        for (int j = 0; j < NT; ++j) dal[j][mt][r] = first[j][mt][r] && topl[mt][r] > 0.f ? g : 0.f;
                    }
                }
            }
            if constexpr (MODE == PT_B1) {
                pt_add_bn_sums<NT, 2>(dal, zl, sv_l, n, h, T, qa, qb);
                continue;
            }
            // ---- B2 / B3
            f32x16 da1[NT][MT1];
            if constexpr (TWO) {
                f32x16 dzl[NT][2];
                pt_dz<NT, 2>(dal, zl, sv_l, bco_l, n, h, T, dzl);
                // dx2 = W2^T dz2: its first 32 rows are y1's cotangent, the other 32 summed over the rows the maximum's
                f32x16 dy1[NT], dtop = zero16();
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) {
                    f32x16 acc[NT];
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[j] = zero16();
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float w = a.W2[(32 * mt + tile_chan(r, h)) * 64 + 32 * jt + n];
#pragma unroll
                            for (int j = 0; j < NT; ++j) acc[j] = mfma32(w, dzl[j][mt][r], acc[j]);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        if (jt == 0) {
                            dy1[j] = acc[j];
                        } else {                            // (dz is 0 on the padding columns, and so is their dx)
#pragma unroll
                            for (int r = 0; r < 16; ++r) dtop[r] += acc[j][r];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
#pragma unroll
                    for (int off = 16; off > 0; off >>= 1) dtop[r] += __shfl_xor(dtop[r], off, 64);
                }
                bool first1[NT][1][16];
                pt_first_max<NT, 1>(y1, top1, n, T, first1);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const bool real = 32 * j + n < T;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = dy1[j][r] + (first1[j][0][r] ? dtop[r] : 0.f);
                        da1[j][0][r] = real && y1[j][0][r] > 0.f ? v : 0.f;
                    }
                }
                if constexpr (MODE == PT_B2) {
                    pt_add_bn_sums<NT, 1>(da1, z1, a.saved, n, h, T, qa, qb);
                    // dW2 = sum over the rows of dz2 (x) [y1 | top1]
                    pt_lds_fence();                         // (the previous pillar's reads are done)
                    pt_to_lds<NT, 2>(dzl, dzs, n, h);
                    pt_to_lds<NT, 1>(y1, xs, n, h);
                    if (n == 0) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) tops[tile_chan(r, h)] = top1[0][r];
                    }
                    pt_lds_fence();
                    const float tb = tops[n];
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        f32x16 wy = zero16(), wt = zero16();
#pragma unroll
                        for (int s = 0; s < 16 * NT; ++s) {
                            const float dzv = dzs[(32 * mt + n) * LD + 2 * s + h];
                            wy = mfma32(dzv, xs[n * LD + 2 * s + h], wy);
                            wt = mfma32(dzv, tb, wt);
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            dw[mt][0][r] += (double)wy[r];
                            dw[mt][1][r] += (double)wt[r];
                        }
                    }
                    continue;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
#pragma unroll
                    for (int mt = 0; mt < MT1; ++mt) da1[j][mt] = dal[j][mt];
                }
            }
            if constexpr (MODE == PT_B3) {
                // dW1 = sum over the rows of dz1 (x) x0 (a padding row's x0 is 0)
                f32x16 dz1[NT][MT1];
                pt_dz<NT, MT1>(da1, z1, a.saved, a.bco, n, h, T, dz1);
                pt_lds_fence();
                pt_to_lds<NT, MT1>(dz1, dzs, n, h);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
#pragma unroll
                    for (int s = 0; s < PT_KS; ++s) xs[(2 * s + h) * LD + 32 * j + n] = in[j][s];
                }
                pt_lds_fence();
#pragma unroll
                for (int mt = 0; mt < MT1; ++mt) {
                    f32x16 w = zero16();
#pragma unroll
                    for (int s = 0; s < 16 * NT; ++s) {
                        const float xv = n < 2 * PT_KS ? xs[n * LD + 2 * s + h] : 0.f;
                        w = mfma32(dzs[(32 * mt + n) * LD + 2 * s + h], xv, w);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) dw[0][mt][r] += (double)w[r];
                }
            }
            }
        }
        // ---- the slice's partial
        if constexpr (MODE == PT_F1 || MODE == PT_F2 || MODE == PT_B1) pt_store_pair<2>(qa, qb, part, 0, 64, n, h);
        if constexpr (MODE == PT_B2) {
            pt_store_pair<1>(qa, qb, part, 4096, 4096 + 32, n, h);     // (layer 1 of a two-layer net: 32 channels)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) part[(32 * mt + tile_chan(r, h)) * 64 + 32 * nt + n] = dw[TWO ? mt : 0][nt][r];
                }
            }
        }
        if constexpr (MODE == PT_B3) {
            if (n < 16) {
#pragma unroll
                for (int mt = 0; mt < MT1; ++mt) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) part[(32 * mt + tile_chan(r, h)) * 16 + n] = dw[0][mt][r];
                }
            }
        }
    }
}

__device__ __forceinline__ double pt_slice_sum(const double* part, int64_t live, int at) {
    double s = 0.0;
    for (int64_t i = 0; i * PT_S < live; ++i) s += part[i * PT_K + at];
    return s;
}

// one thread per channel: the batch statistics, the pack the passes read, the running statistics
__global__ __launch_bounds__(64) void pt_finish_stats_kernel(const double* part, int64_t P, const int64_t* n_pillars, int T,
                                                             int units, const float* gamma, const float* beta, double eps,
                                                             double momentum, float* run_mean, float* run_var, int64_t* tracked,
                                                             float* saved) {
    const int c = threadIdx.x;
    const int64_t live = pt_live(P, n_pillars);
    const double n = (double)(live * T);
    if (c == 0 && tracked) *tracked += 1;
    if (c >= units) {
        saved[c] = saved[64 + c] = saved[128 + c] = saved[192 + c] = 0.f;
        return;
    }
    const double s1 = pt_slice_sum(part, live, c), s2 = pt_slice_sum(part, live, 64 + c);
    const double mean = n > 0 ? s1 / n : 0.0;
    double var = n > 0 ? s2 / n - mean * mean : 0.0;
    var = var > 0 ? var : 0.0;
    const double istd = 1.0 / sqrt(var + eps), scale = (double)gamma[c] * istd;
    saved[c] = (float)mean;
    saved[64 + c] = (float)istd;
    saved[128 + c] = (float)scale;
    saved[192 + c] = (float)((double)beta[c] - mean * scale);
    if (run_mean) {
        const double unbiased = var * (n / (n - 1 > 1 ? n - 1 : 1));
        run_mean[c] = (float)((1.0 - momentum) * (double)run_mean[c] + momentum * mean);
        run_var[c] = (float)((1.0 - momentum) * (double)run_var[c] + momentum * unbiased);
    }
}

__global__ __launch_bounds__(64) void pt_finish_bn_kernel(const double* part, int at_beta, int at_gamma, int64_t P,
                                                          const int64_t* n_pillars, int T, int units, float* dgamma, float* dbeta,
                                                          float* bco) {
    const int c = threadIdx.x;
    const int64_t live = pt_live(P, n_pillars);
    const double n = (double)(live * T);
    if (c >= units) {
        bco[c] = bco[64 + c] = 0.f;
        return;
    }
    const double db = pt_slice_sum(part, live, at_beta + c), dg = pt_slice_sum(part, live, at_gamma + c);
    dbeta[c] = (float)db;
    dgamma[c] = (float)dg;
    bco[c] = n > 0 ? (float)(db / n) : 0.f;
    bco[64 + c] = n > 0 ? (float)(dg / n) : 0.f;
}

// dW (rows, cols) from the partial's [rows][ld] block
__global__ __launch_bounds__(256) void pt_finish_dw_kernel(const double* part, int64_t P, const int64_t* n_pillars, int rows, int cols,
                                                           int ld, float* dW) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    const int64_t live = pt_live(P, n_pillars);
    dW[i] = (float)pt_slice_sum(part, live, (i / cols) * ld + i % cols);
}

struct PtWs {
    double* part;
    float* bco;
};

inline PtWs carve_pt(Carver& c, int64_t P) {
    PtWs w;
    w.part = c.take<double>((size_t)((P + PT_S - 1) / PT_S) * PT_K);
    w.bco = c.take<float>(2 * PT_BCO_LAYER);
    return w;
}

template <int MODE>
void pt_launch(const PtArgs& k, bool two, int T, int64_t max_workgroups, hipStream_t s) {
    const int64_t slices = (k.P + PT_S - 1) / PT_S;
    const int NT = T > 32 ? 2 : 1;
    const int waves = pt_waves(NT);
    const dim3 g(grid_clamp((slices + waves - 1) / waves, 65535 * 16, max_workgroups)), blk(64 * waves);
    const size_t lds = (size_t)waves * pt_wave_floats(NT) * sizeof(float);
    if (two) {
        if (NT == 2) hipLaunchKernelGGL((pt_pass_kernel<MODE, true, 2>), g, blk, lds, s, k);
        else hipLaunchKernelGGL((pt_pass_kernel<MODE, true, 1>), g, blk, lds, s, k);
    } else if constexpr (MODE != PT_F2 && MODE != PT_B2) {
        if (NT == 2) hipLaunchKernelGGL((pt_pass_kernel<MODE, false, 2>), g, blk, lds, s, k);
        else hipLaunchKernelGGL((pt_pass_kernel<MODE, false, 1>), g, blk, lds, s, k);
    }
}

PtArgs pt_args(const dal3_pillar_train_args& a, const PtWs& w) {
    PtArgs k = {};
    k.P = a.P, k.n_pillars = a.n_pillars, k.voxels = a.voxels, k.num_points = a.num_points, k.coords = a.coordinates;
    k.C = a.C, k.T = a.max_points;
    k.vx = a.vx, k.vy = a.vy, k.xo = a.x_offset, k.yo = a.y_offset;
    k.W1 = a.layers[0].weight, k.W2 = a.n_layers == 2 ? a.layers[1].weight : nullptr;
    k.saved = a.saved, k.bco = w.bco;
    k.features = a.features, k.canvas = a.canvas, k.canvas_B = a.canvas_B, k.ny = a.ny, k.nx = a.nx;
    k.grad = a.grad;
    for (int i = 0; i < 4; ++i) k.gs[i] = a.grad_stride[i];
    k.part = w.part;
    return k;
}

}  // namespace

size_t pillar_train_workspace_bytes(int64_t P, int n_layers) {
    (void)n_layers;
    Carver c(nullptr, 0);
    carve_pt(c, P);
    return c.off;
}

hipError_t launch_pillar_train_forward(const dal3_pillar_train_args* args, hipStream_t s) {
    const dal3_pillar_train_args& a = *args;
    hipError_t e;
    if (a.canvas) e = launch_fill_words(a.canvas, (size_t)(a.canvas_B * 64 * a.ny * a.nx), 0, s);
    else e = launch_fill_words(a.features, (size_t)a.P * 64, 0, s);
    if (e != hipSuccess) return e;
    Carver c(a.workspace, a.workspace_bytes);
    const PtWs w = carve_pt(c, a.P);
    const PtArgs k = pt_args(a, w);
    const bool two = a.n_layers == 2;
    for (int l = 0; l < a.n_layers; ++l) {
        if (l == 0) pt_launch<PT_F1>(k, two, a.max_points, a.max_workgroups, s);
        else pt_launch<PT_F2>(k, two, a.max_points, a.max_workgroups, s);
        hipLaunchKernelGGL(pt_finish_stats_kernel, dim3(1), dim3(64), 0, s, w.part, a.P, a.n_pillars, a.max_points,
                           (int)a.layers[l].c_out, a.layers[l].bn_weight, a.layers[l].bn_bias, a.eps, a.momentum[l],
                           a.running_mean[l], a.running_var[l], a.num_batches_tracked[l], a.saved + l * PT_SAVED_LAYER);
    }
    pt_launch<PT_F3>(k, two, a.max_points, a.max_workgroups, s);
    return hipGetLastError();
}

hipError_t launch_pillar_train_backward(const dal3_pillar_train_args* args, hipStream_t s) {
    const dal3_pillar_train_args& a = *args;
    Carver c(a.workspace, a.workspace_bytes);
    const PtWs w = carve_pt(c, a.P);
    const PtArgs k = pt_args(a, w);
    const bool two = a.n_layers == 2;
    const int last = a.n_layers - 1, c_in = a.C + 5, units1 = a.layers[0].c_out;
    pt_launch<PT_B1>(k, two, a.max_points, a.max_workgroups, s);
    hipLaunchKernelGGL(pt_finish_bn_kernel, dim3(1), dim3(64), 0, s, w.part, 0, 64, a.P, a.n_pillars, a.max_points, 64,
                       a.dgamma[last], a.dbeta[last], w.bco + last * PT_BCO_LAYER);
    if (two) {
        pt_launch<PT_B2>(k, two, a.max_points, a.max_workgroups, s);
        hipLaunchKernelGGL(pt_finish_dw_kernel, dim3(16), dim3(256), 0, s, w.part, a.P, a.n_pillars, 64, 64, 64, a.dW[1]);
        hipLaunchKernelGGL(pt_finish_bn_kernel, dim3(1), dim3(64), 0, s, w.part, 4096, 4096 + 32, a.P, a.n_pillars, a.max_points, 32,
                           a.dgamma[0], a.dbeta[0], w.bco);
    }
    pt_launch<PT_B3>(k, two, a.max_points, a.max_workgroups, s);
    hipLaunchKernelGGL(pt_finish_dw_kernel, dim3((units1 * c_in + 255) / 256), dim3(256), 0, s, w.part, a.P, a.n_pillars, units1, c_in,
                       16, a.dW[0]);
    return hipGetLastError();
}
