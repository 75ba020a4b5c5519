// dal3_kernels.h — host-visible views of the packed weights and the kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dal3.h"
#include "dal3_device.h"
#include "dal3_fold.h"

// point tiles (of 32 points) per wave; see profiles/LEDGER_r01_r03.md §4 "register budget"
#ifndef DAL3_ENC_T
#define DAL3_ENC_T 2
#endif
#ifndef DAL3_DEC_T
#define DAL3_DEC_T 1
#endif
#ifndef DAL3_HEAD_T
#define DAL3_HEAD_T 1
#endif

// the fp32 throughput encoder screens conv5 on the fp16 MFMA and recomputes the candidates exactly (dal3_enc_screen.hip);
// 0: the dense kernel for every job (A/B builds: make OUT=... EXTRA=-DDAL3_ENC_SCREEN=0)
#ifndef DAL3_ENC_SCREEN
#define DAL3_ENC_SCREEN 1
#endif

// waves per workgroup of the shared-MLP kernels (waves never cooperate, so this only sets the
// granularity at which the dispatcher refills a CU)
#ifndef DAL3_WG_WAVES
#define DAL3_WG_WAVES 4
#endif

// weight-fragment prefetch depth (fragments of 1 KiB per wave kept in flight), see WRing
#ifndef DAL3_PF
#define DAL3_PF 8
#endif
// MEAN_SIZE_ARR of the reference (tools/static_model.py:17-21), the ONE copy in the library: the decode kernels, the
// criterion kernel and dal3_mean_size() (which the Python side checks against arch.MEAN_SIZE when it loads the library)
#define DAL3_MEAN_SIZE_VALUES 4.8, 1.8, 1.5, 10.0, 2.6, 3.2, 2.0, 1.0, 1.6
__device__ __forceinline__ double mean_size_f64(int sc, int j) {   // MEAN_SIZE_ARR[sc][j], float64 as the reference's table
    constexpr double m[9] = {DAL3_MEAN_SIZE_VALUES};
    return sc == 0 ? (j == 0 ? m[0] : j == 1 ? m[1] : m[2])
                   : sc == 1 ? (j == 0 ? m[3] : j == 1 ? m[4] : m[5]) : (j == 0 ? m[6] : j == 1 ? m[7] : m[8]);
}
#define DAL3_BLOB_TAIL_FLOATS 8192   // 32 KiB: room for a ring's over-read past the last stream

// ---- packed PointNetInstanceSeg (BN folded). A "frag block" is [4 q][64 lanes] float4 x KT k-tiles
// of one 32-row output tile, see dal3_device.h::mma_block_ring. Each kernel reads ONE stream of
// blocks laid out in the order it consumes them:
//   enc_stream  conv2 (64->64) | conv3 (64->64) | conv4 (64->128) | conv5 (128->1024), out-tile major
//   dec_stream  conv2 | dconv1a chunk 0 | { dconv1a chunk c+1 (8 frags), dconv2 chunk c (32 frags) }
//               for c = 0..15 (chunk 16 = zeros) | dconv3 (256->128) | dconv4 (128->128)
// where dconv1a = dconv1 columns 0..63 (the per-point out2 part, one 32-output chunk = 8 fragments)
// and dconv2 is K-major (the 32 fragments that multiply dconv1 chunk c into the 8 output tiles).
struct InsSegW {
    const float* w1;          // first layer [2][2][64]
    const float* b1;          // 64
    const float* b2;
    const float* b3;
    const float* b4;
    const float* b5;          // 1024
    const float* dw1g;        // row-major (512,1024): dconv1 columns 64..1087 (the global-feature part)
    const float* db1;         // 512
    const float* db2;
    const float* db3;
    const float* db4;
    const float* dw5;         // row-major (2,128)
    const float* db5;         // 2
    const f32x4* enc_stream;
    const f32x4* dec_stream;
    const f32x4* lat_stream;  // dconv1a (16 out-tiles x 2 k-tiles) | dconv2 (8 x 16), OUT-TILE major: the latency kernels
                              // (dal3_latency.hip) give each wave whole output tiles; dec_stream interleaves them K-major
    // the screened encoder (dal3_enc_screen.hip, DESIGN.md "Screened conv5"): conv5 three more times
    const float* w5row;       // row-major (1024,128) fp32, folded: one candidate's weights in natural channel order
    const f32x4* w5h;         // fp16 MFMA fragments [32 out-tiles][4 kt][2 s] of 1 KiB, the 16-bit family's layout
    const float* scr_pq;      // (1024,2): eps(c) = X * P_c + Q_c bounds |fp16 score - fp32 chain| for ||x||_2 <= X
    const int32_t* scr_flag;  // nonzero: a folded conv5 weight is not finite in fp16 -> the dense kernel runs
    // the compacted dconv2 of the throughput decoder (dal3_pointmlp.hip, DESIGN.md "Compacted dconv2")
    const float* dw2c;        // dconv2 folded, [k 0..511][row 0..31][out-tile 0..7]: W'[32 mt + row][32 c + tile_chan(r, h)] at
                              // chain index k = 32 c + 2 r + h (chunk, accumulator register, lane half: the dense k order)
    // the same for dconv3 / dconv4, whose live input rows go through a per-wave queue: [k][row 0..31][out-tile 0..3],
    // W'[32 mt + row][32 kt + tile_chan(r, h)] at chain index k = 32 kt + 2 r + h (mlp_layer_ring's k order)
    const float* dw3c;        // k 0..255
    const float* dw4c;        // k 0..127
    const int32_t* dec_flag;  // nonzero: a folded dconv2 / dconv3 / dconv4 weight is not finite or one of their folded biases is -0
                              // -> dense path only
    // dconv1's channels proved dead for a whole crop (DESIGN.md "Crop-dead channels of dconv1")
    const float* dw1c;        // dconv1a folded, [chain index k 0..512][k-half h][32]: the 32 floats a lane of half h holds of row
                              // 32 c + tile_chan(r, h) (k = 32 c + 2 r + h) in the dense fragments, float 4 i + e = column
                              // 32 (i / 4) + tile_chan(4 (i % 4) + e, h); row 512, the null channel, is zeros
    const f32x4* w1h;         // dconv1a as fp16 MFMA fragments [16 out-tiles][2 kt][2 s] of 1 KiB (the layout of w5h)
    const float* prn_pq;      // (512,2): |fp16 score - (fp32 chain from gb - gb)| <= X * P_c + Q_c + 2 K 2^-24 |gb| for ||x2||_2 <= X
    const uint32_t* dec_ident;   // DEC_PLAN_LD words: the plan of a crop with nothing flagged (k, then the null channel)
    const int32_t* prn_flag;  // nonzero: a folded dconv1a weight is not finite in fp16 -> no crop has a plan
};
// dead dconv1 channels from which a crop's tiles take the decoder's compacted body (dal3_pointmlp.hip, where it is measured)
#ifndef DAL3_DEC_MIN_DEAD
#define DAL3_DEC_MIN_DEAD 64
#endif
// a plan's chunk count is rounded up to a multiple of this: 2 (the decoder's chunk loop goes in pairs), or 4 = DAL3_DEC_GROUP
// for A/B builds (no shorter last group; measured slower, profiles/LEDGER_r14.md)
#ifndef DAL3_DEC_PLAN_ROUND
#define DAL3_DEC_PLAN_ROUND 2
#endif
// A crop's dconv1 plan (dec_plan_kernel, dal3_misc.hip): its unflagged chain indices in ascending order, padded with the
// null channel DEC_NULL_K; its term gb gathered to match, in the row order tile_from_channels reads (-1 for the null
// channel); its chunk count (even, >= 2; 0: the crop has no plan and the decoder decides on gb as without one).
#define DEC_PLAN_LD 640       // 16 chunks + the four the decoder's loop reads ahead
#define DEC_NULL_K 512
struct DecPlan {
    const uint32_t* k;        // (B, DEC_PLAN_LD)
    const float* gbc;         // (B, 512)
    const int32_t* nch;       // (B)
};
enum {                        // stream geometry in fragments of 256 floats
    ENC_W2 = 0, ENC_W3 = 16, ENC_W4 = 32, ENC_W5 = 64, ENC_FRAGS = 64 + 512,
    DEC_W2 = 0, DEC_MIX = 16, DEC_MIX_FRAGS = 8 + 16 * 40, DEC_W3 = 16 + 648, DEC_W4 = 16 + 648 + 128,
    DEC_FRAGS = 16 + 648 + 128 + 64,
    LAT_W1A = 0, LAT_W2 = 128, LAT_FRAGS = 128 + 512
};

// Where the fragment packers (launch_pack_weight*) write a layer whose (mt,kt) blocks are consumed in groups of `blocks`
// blocks: group 0 at out + a0, group g >= 1 at out + a1 + (g - 1) * stride (elements of the stream); last >= 0: the last
// group sits at out + last instead. blocks == 0: block after block from out.
struct PackGroups {
    int blocks = 0;
    int64_t a0 = 0, a1 = 0, stride = 0, last = -1;
};

struct FcW {
    const float* w[3];   // row-major (c_out, c_in), BN folded
    const float* b[3];
    int c_in[3], c_out[3], relu[3];
    int n;
};

struct PointHeadW {
    const float* w1;     // first layer [C1/32][KS][64]
    const float* b1;
    const float* b2;
    const float* b3;
    const float* b4;
    const f32x4* stream; // conv2 | conv3 | conv4 fragment blocks, out-tile major, back to back
    FcW fc;
    // the screened conv4 (dal3_head_screen.hip, DESIGN.md "Screened conv4 of the point heads"); heads with conv4 256 -> 512
    // only (static box_est, point_emb), NULL for box_emb
    const float* w4row;       // row-major (512,256) fp32, folded: one candidate's weights in natural channel order
    const f32x4* w4h;         // fp16 MFMA fragments [16 out-tiles][8 kt][2 s] of 1 KiB, the 16-bit family's layout
    const float* scr_pq;      // (512,2): E(c) = X * P_c + Q_c bounds |fp16 score - fp32 chain| for ||x||_2 <= X
    const int32_t* scr_flag;  // nonzero: a folded conv4 weight is not finite in fp16 -> every tile runs the dense layer
};

// ---- 16-bit (bf16 / fp16) packed heads: fp32 first layer, biases and FC; MFMA weights as one stream of
// 1-KiB fragments (512 16-bit elements) per kernel, cut into ring segments (dal3_lp.h)
#define LP_ENC_SEG 32     // fragments per ring segment
#define LP_ENC_SEGS 9     // conv2|conv3|conv4 , then conv5 four out-tiles per segment
#define LP_DEC_SEG 40
#define LP_DEC_SEGS 12    // [conv2, dconv1a(0)] , 8 x [1a(2i+1), 2(2i), 1a(2i+2), 2(2i+1)] , dconv3 x2 , [dconv4, dconv5]
#define LP_HEAD_SEG 32
#ifndef DAL3_LP_ENC_T
#define DAL3_LP_ENC_T 4
#endif
#ifndef DAL3_LP_DEC_T
#define DAL3_LP_DEC_T 2
#endif
#ifndef DAL3_LP_HEAD_T
#define DAL3_LP_HEAD_T 2
#endif
struct InsSegLpW {
    const float* w1;          // fp32 first layer [2][2][64]
    const float* b1;
    const float* bias_enc;    // b2 64 | b3 64 | b4 128 | b5 1024
    const float* bias_dec;    // b2 64 | db2 256 | db3 128 | db4 128 | dw5 (2,128) | db5 (32)
    const float* dw1g;        // fp32 row-major (512,1024)
    const float* db1;         // 512
    const uint16_t* enc_stream;
    const uint16_t* dec_stream;
};
struct PointHeadLpW {
    const float* w1;
    const float* b1;
    const float* bias;        // b2 C2 | b3 C3 | b4 512
    const uint16_t* stream;
    FcW fc;
};
// ---- "f16x3" (dal3_pointmlp_x3.hip): fp16 MFMAs on (hi, lo) split operands, fp32 accuracy. Same blob shape as the 16-bit
// heads (fp32 first layer, biases, FC; one fragment stream), the stream holding a (hi, lo) fragment pair per k-step and
// padded to whole ring segments per group of points.
#ifndef DAL3_X3_HEAD_T
#define DAL3_X3_HEAD_T 2
#endif
#ifndef DAL3_X3_ENC_T
#define DAL3_X3_ENC_T 2
#endif
#ifndef DAL3_X3_DEC_T
#define DAL3_X3_DEC_T 2
#endif
typedef PointHeadLpW PointHeadX3W;
struct InsSegX3W {
    const float* w1;          // fp32 first layer [2][2][64]
    const float* b1;
    const float* bias_enc;    // b2 64 | b3 64 | b4 128 | b5 1024
    const float* bias_dec;    // b2 64 | db2 256 | db3 128 | db4 128 | db5 (32: rows 0, 1 real)
    const float* dw1g;        // fp32 row-major (512,1024): the per-crop part of dconv1
    const float* db1;         // 512
    const uint16_t* enc_stream;   // 18 segments of 32 fragments
    const uint16_t* dec_stream;   // 27 segments
};
hipError_t launch_ins_seg_encode_x3(const InsSegX3W& w, BCN pts, int c_in, int B, int N, float* g, hipStream_t s);
hipError_t launch_ins_seg_decode_x3(const InsSegX3W& w, BCN pts, int c_in, int B, int N, const float* gbias, float* logits,
                                    uint8_t* mask, hipStream_t s);
int point_head_x3_segments(int head_kind);
hipError_t launch_point_head_x3(int head_kind, const PointHeadX3W& w, BCN x, int c_in, int B, int M, float* feat,
                                const int32_t* distinct, hipStream_t s);
// (hi, lo) fragment pairs of a layer, out-tile major: [mt][kt][k-step][hi | lo][64 lanes][8]; element order as
// launch_pack_weight_lp; kt_major: [kt][mt][...] (a K-major layer consumed chunk by chunk)
hipError_t launch_pack_weight_x3(const dal3_layer& L, int kt_major, int col_off, int n_cols, int mt_n, int kt_n, uint16_t* out,
                                 hipStream_t s, PackGroups G = PackGroups{});
hipError_t launch_ins_seg_encode_lp(int dtype, const InsSegLpW& w, BCN pts, int c_in, int B, int N, float* g, hipStream_t s);
hipError_t launch_ins_seg_decode_lp(int dtype, const InsSegLpW& w, BCN pts, int c_in, int B, int N, const float* gbias,
                                    float* logits, uint8_t* mask, hipStream_t s);
hipError_t launch_point_head_lp(int dtype, int head_kind, const PointHeadLpW& w, BCN x, int c_in, int B, int M,
                                float* feat, const int32_t* distinct, hipStream_t s);
// 16-bit fragment packing: element j of lane l of fragment (mt,kt,s) = W'[32mt + (l&31)][32kt + 16s + 8(j>>2) + 4(l>>5) + (j&3)]
hipError_t launch_pack_weight_lp(const dal3_layer& L, int dtype, int kt_major, int col_off, int n_cols, int mt_n, int kt_n,
                                 uint16_t* out, hipStream_t s, PackGroups G = PackGroups{});

// the blobs' layouts (all sections 256-byte aligned) are the walks of dal3_api.hip
void point_head_dims(int head_kind, int* c_in, int* ks, int c[4], int* n_fc, int fc_in[3], int fc_out[3]);

// ---- launchers (all asynchronous on s)
// prune (optional, (B, 513) words, ZERO-FILLED by the caller): the screened encoder leaves there, per crop, the keys of
// U_c = max_p s16(c,p) of dconv1a's fp16 scores (prune_key) and, in word 512, the bits of X = max_p ||x2(p)||_2 (+Inf:
// the crop has no bound). Written only where dec_plan_route() says the screened encoder runs.
hipError_t launch_ins_seg_encode(const InsSegW& w, BCN pts, int c_in, int B, int N, float* g, hipStream_t s, uint32_t* prune = nullptr);
hipError_t launch_ins_seg_encode_screen(const InsSegW& w, BCN pts, int c_in, int B, int N, float* g, hipStream_t s, uint32_t* prune);
bool dec_plan_route(int flags, int B, int N);
int enc_route(int flags, int B, int N);                     // which fp32 encoder runs: DAL3_ENC_ROUTE_* (dal3.h)
bool enc_resident_route(int flags, int B, int N);           // the screened encoder as ONE crop-resident launch (dal3_pointmlp.hip)
bool dec_pair_route(int flags, int B, int N);               // the throughput decoder as pairs of waves (dal3_pointmlp.hip)
int dec_route(int flags, int B, int N, bool guarded);       // which fp32 decoder runs: DAL3_DEC_ROUTE_* (dal3.h)
hipError_t launch_pack_dec_prune(const dal3_layer& L, float* dw1c, float* pq, uint32_t* ident, int32_t* flag, hipStream_t s);
// plan_k (B, DEC_PLAN_LD), plan_gbc (B, 512), plan_nch (B): see DecPlan
hipError_t launch_dec_plan(const InsSegW& w, const float* gb, const uint32_t* prune, int B, uint32_t* plan_k, float* plan_gbc,
                           int32_t* plan_nch, hipStream_t s);
// the bound coefficients (pq) and fp16-range flag of a screened layer: the encoder's conv5 (128 -> 1024) or a head's conv4 (256 -> 512)
hipError_t launch_pack_screen_bound(const dal3_layer& L, float* pq, int32_t* flag, hipStream_t s);
// the chain-ordered copy of dconv2 / dconv3 / dconv4 and its guard; bias: the layer's packed bias (written earlier on s)
hipError_t launch_pack_dec_chain(const dal3_layer& L, const float* bias, float* wcopy, int32_t* flag, hipStream_t s);
hipError_t launch_ins_seg_decode(const InsSegW& w, BCN pts, int c_in, int B, int N, const float* gbias,
                                 float* logits, uint8_t* mask, hipStream_t s, DecPlan plan = DecPlan{nullptr, nullptr, nullptr});
// distinct (B) i32 or NULL: only the first distinct[b] points of item b are distinct (the rest duplicate them)
// feat (B,512) need NOT be initialised: the launchers zero it (NaN rows for items with non-finite inputs) themselves.
// worklist (optional, point_head_worklist_bytes(B, M) bytes of device scratch): lets the throughput family run as
// persistent waves over the compacted list of live tiles (dal3_pointmlp.hip); NULL -> one workgroup per (item, tile)
size_t point_head_worklist_bytes(int B, int M);
hipError_t launch_point_head(int head_kind, const PointHeadW& w, BCN x, int c_in, int B, int M, float* feat,
                             const int32_t* distinct, hipStream_t s, void* worklist = nullptr, size_t worklist_bytes = 0);
// The screened route of launch_point_head (dal3_head_screen.hip): the tiles of `list` (ctl[0] entries, ctl[1] = cursor)
// with conv4 screened against the exact values that the seed launch has left in feat.
// Seed tiles are the live tiles of an item whose index is a multiple of DAL3_HEAD_SCR_STRIDE. Measured at 4096 x 512
// object points, the bench mix of distinct counts (profiles/LEDGER_r10.md): the head takes 3.42 / 3.22 / 3.23 / 3.11 ms
// at 2 / 3 / 4 / 8 against 3.97 ms dense. 8 was the fastest there, but its lists overflow in about 1 % of the tiles (CPU
// model; capacity 1024 holds the model's maximum up to 4) and the dispatch minimum below was swept at 4 only.
#ifndef DAL3_HEAD_SCR_STRIDE
#define DAL3_HEAD_SCR_STRIDE 4
#endif
// 0: the dense persistent kernel for every job (A/B builds: make OUT=... EXTRA=-DDAL3_HEAD_SCREEN=0)
#ifndef DAL3_HEAD_SCREEN
#define DAL3_HEAD_SCREEN 1
#endif
// The screened route is taken from this many 32-point tiles (B * ceil(M / 32)) upward. Measured at stride 4
// (profiles/LEDGER_r10.md, B x 512 object points, bench mix / every point distinct, us dense -> screened): 4096 tiles
// 343 -> 348 / 354 -> 383, 6144 tiles 426 -> 482 / 510 -> 545, 8192 tiles 576 -> 523 / 671 -> 669, 16384 tiles
// 1129 -> 938 / 1376 -> 1325. Below 8192 the second launch and the seed launch's own tail cost more than the screen saves.
#ifndef DAL3_HEAD_SCR_MIN_TILES
#define DAL3_HEAD_SCR_MIN_TILES 8192
#endif
static_assert(DAL3_HEAD_SCR_STRIDE >= 2, "stride 1 leaves no tile to screen");
hipError_t launch_point_head_screen(int head_kind, const PointHeadW& w, BCN x, int c_in, float* feat, uint32_t* ctl,
                                    const u32x4* list, int64_t max_tiles, int64_t slots, hipStream_t s);
// The item-resident route (dal3_head_screen.hip): a workgroup of DAL3_WG_WAVES waves per CU takes whole items from a
// cursor, every live tile screened.
bool head_resident_route(int flags, int head_kind, int B, int M);
int head_route(int flags, int head_kind, int B, int M);    // which point-head kernels run: DAL3_HEAD_ROUTE_* (dal3.h)
hipError_t launch_point_head_resident(int head_kind, const PointHeadW& w, BCN x, int c_in, int B, int M, float* feat,
                                      const int32_t* distinct, hipStream_t s, void* cursor, int cus);
hipError_t launch_pack_head_screen(const dal3_layer& L, float* pq, int32_t* flag, hipStream_t s);
hipError_t launch_generic_layer(const f32x4* wf, const float* w1, const float* bias, int kt_n, int ks_n, int mt_n,
                                int relu, BCN x, int c_in, int B, int N, float* y, hipStream_t s);

// y[b, :c_out] = relu?(W x[b] + bias); x row stride xs, y row stride ys (floats)
hipError_t launch_fc(const float* W, const float* bias, const float* x, int64_t xs, float* y, int64_t ys, int B,
                     int c_in, int c_out, int relu, hipStream_t s);

enum { PACK_FRAG_MT_MAJOR = 0, PACK_FRAG_KT_MAJOR = 1, PACK_FIRST = 2, PACK_ROWMAJOR = 3 };
// G: the fragment modes only (offsets in floats)
hipError_t launch_pack_weight(const dal3_layer& L, int mode, int col_off, int n_cols, int mt_n, int kt_n, float* out,
                              hipStream_t s, PackGroups G = PackGroups{});
hipError_t launch_pack_bias(const dal3_layer& L, float* out, hipStream_t s);

hipError_t launch_static_crop_prep(const double* points, const int64_t* offsets, const int32_t* choice, const double* pose,
                                   const double* box, int B, int N, uint64_t seed, int64_t item_offset, float* pts_out,
                                   float* init_box_out, hipStream_t s);
hipError_t launch_dynamic_item_prep(const double* points, const int64_t* frame_offsets, const double* boxes,
                                    const int64_t* track_first, const int32_t* item_track, const int32_t* item_frame,
                                    const int32_t* choice, const double* pose, int B, int n_per, int r, int s_,
                                    uint64_t seed, int64_t item_offset, float* pts_out, float* box_out,
                                    float* init_box_out, hipStream_t st);
hipError_t launch_static_crop_labels(const double* points, const int64_t* offsets, const int32_t* choice, const double* pose,
                                     int B, int N, uint64_t seed, int64_t item_offset, const double* gt_planes,
                                     uint8_t* mask_label, hipStream_t s);
hipError_t launch_dynamic_item_labels(const double* points, const int64_t* frame_offsets, const int64_t* track_first,
                                      const int32_t* item_track, const int32_t* item_frame, const int32_t* choice,
                                      const double* pose, int B, int n_per, int r, uint64_t seed, int64_t item_offset,
                                      const double* xform, const double* planes, const uint8_t* valid, uint8_t* mask_label,
                                      hipStream_t st);
// dal3_crops.hip
size_t crop_workspace_bytes(int64_t K_total, int64_t max_points_per_frame);
hipError_t launch_crop_count(const float* points, const int64_t* point_offsets, const double* planes,
                             const float* spheres, const int64_t* box_offsets, int F, int64_t K_total, int64_t max_points_per_frame,
                             int64_t* counts, int32_t* cc, hipStream_t s);
hipError_t launch_crop_fill(const float* points, const int64_t* point_offsets, const double* planes,
                            const float* spheres, const int64_t* box_offsets, int F, int64_t K_total,
                            int64_t max_points_per_frame, const double* pose, const int64_t* counts,
                            const int64_t* box_start, const int32_t* cc, double* out_points, int32_t* out_index,
                            int64_t out_capacity, hipStream_t s);
hipError_t launch_crop_starts(const int64_t* counts, const int64_t* order, int64_t K, int64_t* box_start, int64_t* out_offsets,
                              int64_t out_capacity, hipStream_t s);
// rotated-box IoU (dal3_iou.hip): boxes (n,7) / (m,7) [x,y,z,l,w,h,yaw] float32 or float64 (boxes_f64); outputs may be NULL
int64_t box_iou_pairwise_blocks(int64_t n, int64_t m);
int64_t box_iou_paired_blocks(int64_t n);
hipError_t launch_box_iou_pairwise(const void* a, int64_t n, const void* b, int64_t m, int boxes_f64, float* iou_bev,
                                   float* iou_3d, hipStream_t s);
hipError_t launch_box_iou_paired(const void* a, const void* b, int64_t n, int boxes_f64, float* iou_bev, float* iou_3d,
                                 hipStream_t s);
// box-estimation training metrics (dal3_metrics.hip): one launch of 1 + B * chunks(N) blocks (chunks only with logits)
int64_t box_estimation_metrics_chunks(int64_t N);
hipError_t launch_box_estimation_metrics(const dal3_box_metric_args* a, hipStream_t s);
// tracking run (dal3_track.hip)
size_t track_workspace_bytes(int64_t S, int64_t K, int64_t capacity);
size_t track_match_workspace_bytes(int64_t K);
hipError_t launch_track(const dal3_track_args* a, hipStream_t s);
hipError_t launch_track_match(const dal3_track_match_args* a, hipStream_t s);
// motion-state run (dal3_motion.hip)
size_t group_workspace_bytes(int64_t E, int64_t T);
size_t motion_classify_workspace_bytes(int64_t T);
hipError_t launch_group_by_key(const dal3_group_args* a, hipStream_t s);
hipError_t launch_track_features(const dal3_track_feature_args* a, hipStream_t s);
hipError_t launch_gt_table(const dal3_gt_table_args* a, hipStream_t s);
hipError_t launch_motion_classify(const dal3_motion_classify_args* a, hipStream_t s);
// baseline runs (dal3_score.hip): one slab entry per 256-sample chunk; the second stage is a launch of its own
size_t score_workspace_bytes(int64_t S);
hipError_t launch_score_tracks(const dal3_score_args* a, hipStream_t s);
hipError_t launch_best_gt_iou(const dal3_best_gt_args* a, hipStream_t s);
// detector post-processing (dal3_nms.hip): sort + suppress, one workgroup per segment; count / scan / fill of the decode
size_t nms_workspace_bytes(int64_t K, int boxes_f64);
hipError_t launch_nms(const dal3_nms_args* a, hipStream_t s);
size_t center_decode_workspace_bytes(int64_t B, int64_t H, int64_t W);
hipError_t launch_center_decode(const dal3_center_decode_args* a, hipStream_t s);
// double_flip: the four views' un-flip, merge and decode in the same three launches; DoubleFlip's copies of the points
hipError_t launch_center_decode_flip4(const dal3_center_decode_flip4_args* a, hipStream_t s);
hipError_t launch_flip4_points(const float* points, int64_t N, int C, const int64_t* offsets, int64_t B, float* out,
                               int64_t* out_offsets, int64_t max_workgroups, hipStream_t s);
// the Waymo sweep merge of LoadPointCloudFromFile (dal3_sweeps.hip): raw planes -> the voxeliser's rows, one launch a batch
hipError_t launch_sweep_merge(const dal3_sweep_segment* segments, int64_t B, int nsweeps, int64_t N, float* out,
                              int64_t* point_offsets, int64_t max_workgroups, hipStream_t s);
// the PointPillars reader (dal3_pillars.hip): voxelisation as a stable radix sort over chunks, the fused feature kernel
size_t voxelize_workspace_bytes(int64_t B, int64_t N);
hipError_t launch_voxelize(const dal3_voxelize_args* a, hipStream_t s);
hipError_t launch_pillar_pack(const dal3_layer* layers, int n_layers, double eps, float* out, hipStream_t s);
hipError_t launch_pillar_features(const dal3_pillar_feature_args* a, hipStream_t s);
hipError_t launch_pillar_scatter(const float* features, const int32_t* coordinates, int64_t P, const int64_t* n_pillars, int c_out,
                                 float* canvas, int64_t canvas_B, int64_t ny, int64_t nx, hipStream_t s);
hipError_t launch_voxel_mean(const float* voxels, const int32_t* num_points, int64_t P, const int64_t* n_pillars, int max_points,
                             int C, float* out, hipStream_t s);
// ... and its training step (dal3_pillars_train.hip); the arguments are checked by the caller
size_t pillar_train_workspace_bytes(int64_t P, int n_layers);
hipError_t launch_pillar_train_forward(const dal3_pillar_train_args* a, hipStream_t s);
hipError_t launch_pillar_train_backward(const dal3_pillar_train_args* a, hipStream_t s);
// the detector's dense stage (dal3_conv2d.hip): 3x3 / 1x1 / transposed convolutions as one implicit GEMM on the fp32 MFMA
size_t conv2d_pack_floats(int kind, int c_in, int c_out);
// (internal: any c_in / c_out the format can hold, not only the public entry's 4096; the RoI head packs its sections here)
hipError_t launch_conv2d_pack(const FoldLayer& layer, int kind, float* out, hipStream_t s);
hipError_t launch_conv2d(const dal3_conv2d_args* a, hipStream_t s);
// ... and on 16-bit MFMA operands (dal3_conv2d_lp.hip); dtype DAL3_F16 or DAL3_BF16, checked by the caller
size_t conv2d_lp_pack_bytes(int kind, int c_in, int c_out);
hipError_t launch_conv2d_lp_pack(const FoldLayer& layer, int kind, int dtype, void* out, hipStream_t s);
hipError_t launch_conv2d_lp(const dal3_conv2d_lp_args* a, hipStream_t s);
// ... and their backward pass (dal3_conv2d_train.hip); the arguments are checked by the caller
size_t conv2d_dgrad_pack_floats(int kind, int c_in, int c_out);
hipError_t launch_conv2d_dgrad_pack(const float* weight, int kind, int c_in, int c_out, float* out, hipStream_t s);
hipError_t launch_conv2d_dgrad(const dal3_conv2d_dgrad_args* a, hipStream_t s);
size_t conv2d_wgrad_workspace_bytes(int kind, int stride, int c_in, int c_out, int64_t B, int64_t H, int64_t W);
hipError_t launch_conv2d_wgrad(const dal3_conv2d_wgrad_args* a, hipStream_t s);
// the VoxelNet detector's sparse 3-D middle (dal3_spconv.hip): site bookkeeping on the chunked radix sort, gather-GEMM convolutions
size_t sp_sort_workspace_bytes(int64_t capacity);
hipError_t launch_sp_sort(const dal3_sp_sort_args* a, hipStream_t s);
int sp_candidates(const int32_t* kernel, const int32_t* stride);
size_t sp_downsample_workspace_bytes(int64_t in_capacity, int candidates);
hipError_t launch_sp_downsample(const dal3_sp_downsample_args* a, hipStream_t s);
hipError_t launch_sp_table(const dal3_sp_table_args* a, hipStream_t s);
size_t sp_conv_pack_floats(int taps, int c_in, int c_out);
hipError_t launch_sp_conv_pack(const FoldLayer& layer, int taps, float* out, int32_t* status, hipStream_t s);
hipError_t launch_sp_conv(const dal3_sp_conv_args* a, hipStream_t s);
// ... and its convolutions on 16-bit MFMA operands (dal3_spconv_lp.hip); dtype DAL3_F16 or DAL3_BF16, checked by the caller
size_t sp_conv_lp_pack_bytes(int taps, int c_in, int c_out);
hipError_t launch_sp_conv_lp_pack(const FoldLayer& layer, int taps, int dtype, void* out, int32_t* status, hipStream_t s);
hipError_t launch_sp_conv_lp(const dal3_sp_conv_lp_args* a, hipStream_t s);
hipError_t launch_sp_table_transposed(const dal3_sp_table_transposed_args* a, hipStream_t s);
size_t sp_wgrad_workspace_bytes(int taps, int c_in, int c_out, int64_t out_capacity);
hipError_t launch_sp_wgrad(const dal3_sp_wgrad_args* a, hipStream_t s);
hipError_t launch_points_in_boxes(const void* points, int points_f64, int64_t P, int64_t stride, const double* planes,
                                  int K, int f32_math, uint8_t* inside, hipStream_t s);
hipError_t launch_writeback(const double* final_boxes, const int32_t* final_idx, const double* pose_best,
                            const double* pose_inv, const double* track_box, float* det, const int64_t* det_start,
                            const int32_t* det_count, const uint8_t* active, int P, int64_t n_det, int32_t* match,
                            int32_t* owner, hipStream_t s);
hipError_t launch_maxpool_n(const void* x, int dtype, int64_t rows, int64_t n, void* out, hipStream_t s);
hipError_t launch_segment_counts(const uint8_t* mask, int B, int N, int32_t* counts, hipStream_t s);
// p[0..n_words) = value (32-bit words) as a kernel launch; used instead of hipMemsetAsync wherever the call may be
// captured into a hipGraph (see dal3_misc.hip)
hipError_t launch_fill_words(void* p, size_t n_words, uint32_t value, hipStream_t s);
// dst (B, C) = 0, or the quiet-NaN pattern in the rows of items whose input x (B, c_in, n_pts) holds a NaN / Inf
// distinct / worklist (optional): also build the point heads' worklist (ctl at worklist, entries at worklist + 256);
// seed_stride > 0: as two lists, the seed tiles and the others (the screened heads, dal3_head_screen.hip)
hipError_t launch_nonfinite_rows(BCN x, int B, int n_pts, int c_in, float* dst, int C, hipStream_t s,
                                 const int32_t* distinct = nullptr, void* worklist = nullptr, int seed_stride = 0);
hipError_t launch_compact_sample(const uint8_t* mask, BCN pts, int B, int N, int C, int M, int sampler,
                                 const int32_t* choice, uint64_t seed, int64_t item_offset, int32_t* counts,
                                 int32_t* pos, int32_t* obj_idx, float* obj_pts, hipStream_t s, const int64_t* step = nullptr);
// arguments of the box decode (dal3_decode_boxes of include/dal3.h), also taken by the fused last-FC + decode launch
struct DecodeArgs {
    float* box_pred;
    const float* center_add;
    int64_t ca_stride;
    int center_inplace;
    const float* boxes_center_add;
    int64_t bca_stride;
    const float* yaw_base;
    int64_t yaw_stride;
    float* heading_residuals;
    float* size_residuals;
    float* center;
    float* boxes7;
};
// box_pred (B,39) = W (39, c_in) x + bias, then the decode of those rows, one launch; box_pred = d.box_pred
hipError_t launch_fc39_decode(const float* W, const float* bias, const float* x, int64_t xs, int B, int c_in,
                              const DecodeArgs& d, hipStream_t s);
hipError_t launch_decode_boxes(float* box_pred, int B, const float* center_add, int64_t center_add_stride,
                               int center_inplace, const float* boxes_center_add, int64_t boxes_center_add_stride,
                               const float* yaw_base, int64_t yaw_stride, float* heading_residuals,
                               float* size_residuals, float* center, float* boxes7, hipStream_t s);
hipError_t launch_recenter(const float* obj_pts, int B, int M, const float* init_box7, const float* box_one7,
                           const float* bbox_gt7, float* obj_pts_two, int64_t* hcl, float* hrl, hipStream_t s);

// dal3_train.hip: training-mode building blocks over point-major (M x C) fp32 activations
hipError_t launch_tr_linear(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                            int relu_in, const float* W, int64_t ldw, int transpose_w, const float* bias, int64_t seg,
                            int c_out, float* z, int64_t ldz, int accumulate, float* ws, hipStream_t s, bool prepacked = false);
size_t tr_linear_workspace_bytes(int c_in, int c_out);
// the fragment layout (output tiles per wave) launch_tr_linear will read for this shape, 0: it packs nothing
int tr_linear_pack_mtb(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, int has_act);
hipError_t launch_tr_pack_many(const dal3_tr_pack_item* items, int n, hipStream_t s);
// the training forward's big layers on the f16x3 engine (dal3_train_x3.hip): layout code 0x100 | MTB, or 0 when the call
// does not qualify (then it takes launch_tr_linear)
int tr_linear_x3_layout(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, int has_act);
hipError_t launch_tr_linear_x3(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift, int relu_in,
                               const uint16_t* wpk, int layout, const float* bias, int64_t seg, int c_out, float* z, int64_t ldz,
                               hipStream_t s, const uint32_t* in_amax = nullptr);
size_t tr_colred_workspace_bytes(int64_t M, int C);
hipError_t launch_tr_act_colsum(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift, int relu,
                                float* out, int64_t ldo, double* part, double* sums, hipStream_t s);
hipError_t launch_tr_colred(const float* z, int64_t M, int C, int64_t ldz, int mode, const float* da, int64_t ldda,
                            const float* dg, const int32_t* arg, int64_t seg, const float* scale, const float* shift,
                            const float* mu, const float* rstd, double* part, double* out, hipStream_t s);
hipError_t launch_tr_pool_coef(const float* dg, const float* g, const float* zarg, const float* mu, const float* rstd,
                               const float* gamma, int B, int C, int64_t M, double* coef, float* kd, hipStream_t s);
hipError_t launch_tr_pool_moments(const float* W, int64_t ldw, const float* b, const double* m1, const float* Sc, int64_t M, int C,
                                  int K, double* sums, hipStream_t s);
// the shapes the moment-route kernels / the conv1 kernels are built for (dal3_train.hip), for the C ABI's argument checks
// (hidden: the library's exported names stay the C ABI's and the launchers')
__attribute__((visibility("hidden"))) bool tr_pool_k_ok(int K);
__attribute__((visibility("hidden"))) bool tr_conv1_ok(int c_in, int c_out);
size_t tr_pool_gv_workspace_bytes(int K);
hipError_t launch_tr_pool_gv(const double* coef, const float* W, int64_t ldw, const float* b, int C, int K, float* G, float* v,
                             double* ws, hipStream_t s);
hipError_t launch_tr_pool_dw(const double* coef, const float* W, int64_t ldw, const float* b, const float* S, const double* m1,
                             int64_t M, int centred, const float* dWs, int C, int K, float* dW, hipStream_t s);
// the 128 -> 2 logits layer with its Dropout as VALU kernels (dal3_train.hip)
hipError_t launch_tr_head2_forward(const float* z, int64_t M, int64_t ldz, const float* scale, const float* shift, int relu,
                                   const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop, const float* W,
                                   int64_t ldw, const float* bias, float* logits, hipStream_t s);
hipError_t launch_tr_head2_dgrad(const float* dl, int64_t M, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step,
                                 float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda, hipStream_t s);
hipError_t launch_tr_head2_dgrad_bnbwd(const float* dl, int64_t M, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step,
                                       float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda, const float* bz,
                                       int64_t ldbz, const float* bscale, const float* bshift, const float* bmu, const float* brstd,
                                       const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3, double* part,
                                       hipStream_t s);
size_t tr_head2_wgrad_workspace_bytes(int64_t M);
hipError_t launch_tr_head2_wgrad(const float* dl, const float* z, int64_t M, int64_t ldz, const float* scale, const float* shift,
                                 int relu, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop,
                                 double* ws, float* dWb, hipStream_t s);
// the first layer of a stack (c_in <= 8) as VALU kernels (dal3_train.hip)
hipError_t launch_tr_wgrad_final_many(const dal3_tr_wgrad_part* items, int n, hipStream_t s);
hipError_t launch_parse_box_pred(const float* bp, int64_t ldb, int B, float* c, float* hs, float* hrn, float* hr, float* ss, float* srn,
                                 float* sr, hipStream_t s);
hipError_t launch_parse_box_pred_backward(const float* gc, const float* ghs, const float* ghrn, const float* ghr, const float* gss,
                                          const float* gsrn, const float* gsr, int B, float* g, hipStream_t s);
// dal3_train_fc.hip
int tr_fc_max_rows();
int tr_fc_max_act_cin();
hipError_t launch_tr_fc_forward(const float* a, int B, int c_in, int64_t lda, const float* in_scale, const float* in_shift, int relu_in,
                                const float* W, int64_t ldw, int transpose_w, const float* bias, int c_out, float* z, int64_t ldz,
                                const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                                float eps, float* mu, float* rstd, float* scale, float* shift, hipStream_t s);
hipError_t launch_tr_fc_backward_w(const float* da, int64_t ldda, int B, int c_out, const float* z, int64_t ldz, const float* scale,
                                   const float* shift, const float* mu, const float* rstd, const float* gamma, float* dgamma,
                                   float* dbeta, const float* a_prev, int c_in, int64_t lda, const float* in_scale,
                                   const float* in_shift, int relu_in, float* dz, int64_t lddz, float* dW, int64_t lddw, float* db,
                                   hipStream_t s);
size_t tr_conv1_workspace_bytes(int64_t Mp, int c_out);
hipError_t launch_tr_conv1_bn_stats(const float* x, int64_t M, int64_t Mp, int c_in, int64_t ldx, const float* W, int64_t ldw,
                                    const float* bias, int c_out, float* z, int64_t ldz, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                    float* scale, float* shift, double* part, hipStream_t s);
hipError_t launch_tr_conv1_wgrad(const float* dz, int64_t lddz, const float* x, int64_t M, int c_in, int64_t ldx, int c_out, double* part,
                                 float* dW, hipStream_t s);
hipError_t launch_tr_gather_at(const float* z, int64_t ldz, const int32_t* arg, int64_t seg, int n_seg, int C, float* out, hipStream_t s);
hipError_t launch_tr_pool_zarg(const int32_t* arg, const float* a, int64_t lda, const float* W, int64_t ldw, const float* bias, int B,
                               int C, int K, int N, float* zarg, hipStream_t s);
hipError_t launch_tr_pool_sparse(const int32_t* arg, const float* kd, const float* W, int64_t ldw, const float* a, int64_t lda,
                                 int B, int C, int K, int N, float* da, int64_t ldda, float* dWs, hipStream_t s);
hipError_t launch_tr_box_loss(const float* center, const float* center_label, const float* hs, const float* hrn,
                              const int64_t* hcl, const float* hrl, const float* ss, const float* srn, const int64_t* scl,
                              const float* srl, int B, float* losses, float* g_center, float* g_hs, float* g_hrn, float* g_ss,
                              float* g_srn, hipStream_t s);
size_t tr_seg_ce_workspace_bytes(int64_t M);
hipError_t launch_tr_seg_ce(const float* logits, const void* labels, int labels_i64, int64_t M, float* loss, float* dlogits,
                            double* part, hipStream_t s);
// linear + a column reduction of its output in the kernel's epilogue (dal3_train.hip, TrRed)
size_t tr_linear_red_workspace_bytes();
hipError_t launch_tr_linear_bn_stats(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                     int relu_in, const float* W, int64_t ldw, const float* bias, int64_t seg, int c_out,
                                     float* z, int64_t ldz, float* packed, int64_t rows, const float* gamma, const float* beta,
                                     float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                     float* bn_scale, float* bn_shift, double* part, hipStream_t s, int* fused);
hipError_t launch_tr_linear_bnbwd_sums(const float* a, int64_t M, int c_in, int64_t lda, const float* W, int64_t ldw, int c_out,
                                       float* da, int64_t ldda, float* packed, int64_t rows, const float* bz, int64_t ldbz,
                                       const float* bscale, const float* bshift, const float* bmu, const float* brstd,
                                       const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3,
                                       double* part, hipStream_t s, int* fused);
hipError_t launch_tr_bn_stats(const float* z, int64_t M, int C, int64_t ldz, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                              float* scale, float* shift, double* part, hipStream_t s);
hipError_t launch_tr_bnbwd_sums(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda, const float* dg,
                                const int32_t* arg, int64_t seg, const float* scale, const float* shift, const float* mu,
                                const float* rstd, const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2,
                                float* k3, double* part, hipStream_t s);
hipError_t launch_tr_bn_finalize(const double* sums, int C, int64_t M, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                 float* scale, float* shift, hipStream_t s);
hipError_t launch_tr_bnbwd_coef(const double* sums, int C, int64_t M, const float* gamma, const float* rstd, float* dgamma,
                                float* dbeta, float* k1, float* k2, float* k3, hipStream_t s);
hipError_t launch_tr_bnbwd_apply(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                 const float* dg, const int32_t* arg, int64_t seg, const float* scale, const float* shift,
                                 const float* mu, const float* rstd, const float* k1, const float* k2, const float* k3,
                                 float* dz, int64_t lddz, hipStream_t s, uint32_t* amax = nullptr);
size_t tr_bnbwd_apply_segsum_workspace_bytes(int64_t M, int C);
hipError_t launch_tr_bnbwd_apply_segsum(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                        const float* scale, const float* shift, const float* mu, const float* rstd,
                                        const float* k1, const float* k2, const float* k3, float* dz, int64_t lddz,
                                        int64_t sum_seg, float* seg_sums, double* ws, hipStream_t s);
size_t tr_wgrad_workspace_bytes(int64_t M, int c_out, int c_in);
hipError_t launch_tr_wgrad(const float* dz, int64_t lddz, const float* a, int64_t lda, const float* scale,
                           const float* shift, int relu_in, int64_t M, int c_out, int c_in, float* part, float* dW,
                           hipStream_t s);
hipError_t launch_tr_linear_pool(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                 int relu_in, const float* W, int64_t ldw, const float* bias, const float* out_scale,
                                 const float* out_shift, int64_t seg, int c_out, float* g, int32_t* arg, float* ws,
                                 unsigned long long* packed, hipStream_t s);
// wgrad on the f16x3 engine (dal3_train_x3.hip): ok -> the layer's shape qualifies; the workspace holds its slices' partial sums
bool tr_wgrad_x3_ok(int64_t M, int c_out, int c_in);
size_t tr_wgrad_x3_workspace_bytes(int64_t M, int c_out, int c_in);
hipError_t launch_tr_wgrad_x3(const float* dz, int64_t lddz, const float* a, int64_t lda, const float* scale, const float* shift,
                              int relu_in, const uint32_t* dz_amax, int64_t M, int c_out, int c_in, float* part, float* dW,
                              hipStream_t s);
hipError_t launch_tr_segmax_unpack(const unsigned long long* packed, int64_t total, float* g, int32_t* arg, hipStream_t s);
bool tr_linear_pool_x3_ok(int64_t M, int c_in, int64_t seg, int c_out);
hipError_t launch_tr_linear_pool_x3(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                    int relu_in, const float* W, int64_t ldw, const float* bias, const float* out_scale,
                                    const float* out_shift, int64_t seg, int c_out, float* g, int32_t* arg, float* ws,
                                    unsigned long long* packed, hipStream_t s);
// A persistent kernel's workgroup w walks the groups w, w + G, w + 2G, ... Workgroup ids are dealt round-robin over the 8
// XCDs (an L2 each), so consecutive groups — the groups of ONE crop, which share the crop's 2-KiB dconv1 term — land on
// different XCDs and each L2 fetches the term for itself. With this virtual id XCD x (ids = x mod 8) owns the
// contiguous virtual blocks [x G/8, (x+1) G/8): a crop's groups of one round share an L2 (round 6; a bijection on [0, G),
// so every group is still walked exactly once; G not a multiple of 8: the plain id).
#if defined(__HIPCC__)
__device__ __forceinline__ int xcd_contiguous_block() {
    const unsigned g = gridDim.x, b = blockIdx.x;
    return (g & 7u) ? (int)b : (int)((b & 7u) * (g >> 3) + (b >> 3));
}
#endif
// small jobs: one 16-wave workgroup per 32-point tile, activations through LDS (dal3_latency.hip); bit-identical results
hipError_t launch_ins_seg_encode_lat(const InsSegW& w, BCN pts, int c_in, int B, int N, float* g, hipStream_t s);
hipError_t launch_ins_seg_decode_lat(const InsSegW& w, BCN pts, int c_in, int B, int N, const float* gbias, float* logits,
                                     uint8_t* mask, hipStream_t s);
hipError_t launch_point_head_lat(int head_kind, const PointHeadW& w, BCN x, int c_in, int B, int M, float* feat,
                                 const int32_t* distinct, hipStream_t s);
bool lat_use(int64_t tiles, int flags, int64_t max_tiles);    // the dispatch rule (dal3_pointmlp.hip)
hipError_t launch_tr_act_dropout(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift, int relu,
                                 const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop, float* out,
                                 int64_t ldo, hipStream_t s);
hipError_t launch_tr_segmax(const float* z, int64_t ldz, int64_t seg, int C, const float* scale, const float* shift,
                            float* g, int32_t* arg, int64_t n_seg, unsigned long long* packed, hipStream_t s);
hipError_t launch_tr_segsum(const float* x, int64_t ldx, int64_t seg, int C, float* out, int64_t n_seg, hipStream_t s);
// CenterPoint's second stage (dal3_roi.hip): BEV point features, the RoI head's fused MLP and box prediction
hipError_t launch_bev_gather(const dal3_bev_gather_args* a, hipStream_t s);
hipError_t launch_box_points(const float* boxes, int64_t n, int cols, int num_point, float* out, hipStream_t s);
size_t roi_pack_floats(const dal3_roi_shape* shape);
int roi_layers(const dal3_roi_shape* shape);
void roi_layer_dims(const dal3_roi_shape* shape, int i, int* c_in, int* c_out);
hipError_t launch_roi_pack(const dal3_roi_shape* shape, const dal3_layer* layers, const double* eps, float* out, hipStream_t s);
size_t roi_head_workspace_bytes(int64_t B, int64_t M, int num_point, int C, int code_size);
hipError_t launch_roi_post(const float* box_preds, const float* cls_preds, const float* roi_scores, int64_t n, int code_size,
                           float* out_boxes, float* out_scores, hipStream_t s);
bool launch_roi_head(const dal3_roi_head_args* a, hipStream_t s, hipError_t* err);
// the second stage's training (dal3_roi_train.hip): target assignment, the RoI losses and their gradients
hipError_t launch_roi_targets(const dal3_roi_targets_args* a, hipStream_t s);
hipError_t launch_roi_loss(const float* rcnn_cls, const float* rcnn_reg, int64_t N, int code_size, const float* cls_labels,
                           const int32_t* reg_valid, const float* gt_of_rois, const float* code_weights, float cls_weight,
                           float reg_weight, float* loss, float* d_cls, float* d_reg, hipStream_t s);
// the first stage's training (dal3_center_loss.hip): AssignLabel's targets, the head's loss and its gradients
hipError_t launch_center_targets(const dal3_center_targets_args* a, hipStream_t s);
size_t center_loss_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
bool launch_center_loss(const dal3_center_loss_args* a, hipStream_t s, hipError_t* err);
// the training input (dal3_augment.hip): GT paste selection, the points' augmentation and shuffle, the boxes' side
hipError_t launch_gt_paste_select(const dal3_gt_paste_args* a, hipStream_t s);
size_t augment_points_workspace_bytes(int64_t B, int64_t n);
bool launch_augment_points(const dal3_augment_points_args* a, hipStream_t s, hipError_t* err);
hipError_t launch_augment_boxes(const dal3_augment_boxes_args* a, hipStream_t s);
// the optimiser step (dal3_optim.hip): the gradients' sum of squares per span, the fused clip + decay + Adam update
int64_t optim_partials(int64_t n_flat);
hipError_t launch_optim_grad_norm(const float* grad, int64_t n_flat, dal3_optim_hyper* hyper, double* partials, hipStream_t s);
hipError_t launch_optim_step(const dal3_optim_chunk* chunks, int64_t n_chunks, float* grad, float* exp_avg, float* exp_avg_sq,
                             int64_t n_flat, const double* partials, dal3_optim_hyper* hyper, hipStream_t s);
hipError_t launch_optim_total_norm(const double* partials, int64_t n_partials, float* out, hipStream_t s);
