/* dal3.h — C ABI of lib3dal_hip.so: the MI355X (gfx950) implementation of the 3DAL
 * Frustum-PointNet auto-labeling heads (eval-mode forward + box decode).
 *
 * Boundary contract:
 *   - plain C, no torch types, no C++ mangling; every pointer is a raw DEVICE pointer unless a
 *     parameter says "host"; the caller (the PyTorch caching allocator, via tensor.data_ptr())
 *     owns every buffer including the workspace and the packed weights;
 *   - every call is asynchronous on the given HIP stream; the library never synchronises the
 *     device, allocates nothing persistent and keeps no mutable global state except a
 *     thread-local error string;
 *   - return 0 on success, a negative DAL3_E* code on failure; dal3_last_error() describes it.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * jacky121298/3DAL_PyTorch checkout).
 */
#ifndef DAL3_H
#define DAL3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dal3_stream;               /* hipStream_t */

#define DAL3_VERSION 170                 /* 0.1.7 (+ dal3_group_by_key / dal3_track_features / dal3_gt_table / dal3_motion_classify and their argument structs, DAL3_MOTION_BAD_KEY: additions only, as dal3_track was; + dal3_track / dal3_track_match, dal3_track_args / dal3_track_match_args, DAL3_TRACK_*: additions only, the number is pinned by the existing tests): dal3_box_estimation_metrics (dal3_box_metric_args / dal3_box_metric_acc); 0.1.6: dal3_box_iou_pairwise / dal3_box_iou_paired; 0.1.5: dal3_crop_starts_capped; upper bounds on B, N (DAL3_MAX_*); DAL3_BCN_NO_LDS_SAMPLER; 0.1.4: dal3_crop_starts, dal3_crop_fill takes out_capacity; 0.1.3: dal3_bcn.flags (DAL3_BCN_*); dal3_tr_linear_bn_stats / dal3_tr_linear_bnbwd_sums; .1: dal3_tr_fc_*, dal3_tr_wgrad_final_many, dal3_parse_box_pred* */

enum {
    DAL3_OK = 0,
    DAL3_EINVAL = -1,                    /* bad shape / stride / alignment / null pointer */
    DAL3_EWORKSPACE = -2,                /* workspace too small */
    DAL3_EHIP = -3                       /* a HIP runtime call failed (message has hipGetErrorString) */
};

/* Upper bounds of ONE call's batch, checked by every entry that takes (B, N) or (B, M) before anything is carved or
 * launched: a call beyond them returns DAL3_EINVAL ("split the batch"). The kernels index an item's points and the
 * per-item outputs with 32-bit ints and launch one workgroup (or worklist entry) per 32-point tile of an item, so a
 * larger job would get a truncated grid or a wrapped offset instead of an error. None of them is reachable with buffers
 * that fit the 288 GB of an MI355X except through a wrong argument: 2^31 tiles of fp32 xyz points alone are 824 GB. */
#define DAL3_MAX_ITEMS 16777216            /* B  <= 2^24 items (crops / track-frames) per call */
#define DAL3_MAX_POINTS_PER_ITEM 16777216  /* N, M, n_box <= 2^24 points per item */
#define DAL3_MAX_TILES 2147483647          /* B * ceil(N / 32) <= 2^31 - 1 (the launch grid) */

/* arithmetic dtype of the shared-MLP kernels of a packed head. DAL3_F32: exact-fp32 MFMA (the reference's
 * precision). DAL3_BF16 / DAL3_F16: weights and inter-layer activations rounded to 16 bits, fp32 accumulate,
 * v_mfma_f32_32x32x16_{bf16,f16} (BASELINE.json configs C3 / C5); dconv5 (128 -> 2) runs as one more 16-bit
 * out-tile of the decode stack; first layer, the per-crop term of dconv1, FC heads, mask and all I/O stay fp32.
 * tests/emu16.py is the reference model of this arithmetic: the kernels' error against the fp32 oracle equals the
 * model's to a few per cent (rms), and the tests hold them to 1.5 x (max) / 1.15 x (rms) of it. The same dtype must be given to dal3_pack_weights and to the forward calls. */
enum { DAL3_F32 = 0, DAL3_BF16 = 1, DAL3_F16 = 2,
       /* fp16 MFMAs on (hi, lo) SPLIT operands: x = x_hi + x_lo, w = w_hi + w_lo in fp16, w x ~ w_hi x_hi + w_hi x_lo + w_lo x_hi,
        * fp32 accumulate — fp32 ACCURACY (logits ~1e-6 of their range, like DAL3_F32) from three fp16 MFMAs per fp32 one.
        * An arithmetic dtype of packed weights only (never a storage dtype of dal3_bcn / dal3_maxpool_n_dtype).
        * Range: folded weights and every layer's activations must stay below fp16's largest finite value (65504) in
        * magnitude. A folded WEIGHT beyond it is packed as NaN — and a binding should refuse it outright at packing
        * time (3dal_pytorch_amd/_hip.py check_f16x3_range raises: the shared-MLP kernels are built without NaN semantics,
        * so a NaN weight is not guaranteed to surface). An ACTIVATION beyond it saturates in the split and the crop's
        * outputs are WRONG WITHOUT NOTICE (DAL3_F32 has no such limit; DAL3_F16 turns NaN there). The margin is three orders of magnitude on this path: the first layer, which sees
        * the raw coordinates, runs in fp32, and crops scaled 1,000 x (box-frame coordinates of kilometres) still match
        * DAL3_F32 to 1e-6 (tests/test_gpu_x3.py). Values below fp16's normal range lose nothing that fp32 accumulation
        * would keep. */
       DAL3_F16X3 = 3 };

/* which sub-network a packed-weight blob belongs to */
enum {
    DAL3_HEAD_INS_SEG = 0,               /* PointNetInstanceSeg: 10 layers, c_in 3 (static) or 4 (dynamic) */
    DAL3_HEAD_STATIC_BOX_EST = 1,        /* static PointNetEstimation: 4 conv + 3 fc */
    DAL3_HEAD_POINT_EMB = 2,             /* PointEmbedding: 4 conv + 2 fc */
    DAL3_HEAD_BOX_EMB = 3,               /* BoxEmbedding: 4 conv + 2 fc */
    DAL3_HEAD_DYNAMIC_BOX_EST = 4        /* dynamic PointNetEstimation: 3 fc */
};

/* how the M object points of a crop are drawn from its segmented points
 * (replaces gather_object_pts, tools/static_model.py:23-49) */
enum {
    DAL3_SAMPLER_DEVICE = 0,             /* counter-based RNG keyed on (seed, global item index, point) */
    DAL3_SAMPLER_CHOICE = 1              /* caller supplies `choice` (B,M): positions into the ordered
                                            list of segmented points, e.g. NumPy's legacy stream drawn
                                            in the reference's order for bit-reproducible eval runs */
};

/* One Conv1d(k=1)/Linear layer with its optional eval-mode BatchNorm1d, as the reference's
 * state_dict holds it: weight (c_out, c_in[,1]) row-major, the rest (c_out). bn_* all NULL => no BN. */
typedef struct {
    const float* weight;
    const float* bias;
    const float* bn_weight;
    const float* bn_bias;
    const float* bn_mean;
    const float* bn_var;
    int32_t c_in;
    int32_t c_out;
} dal3_layer;

/* ------------------------------------------------------------------------------------------ */
int dal3_version(void);
const char* dal3_last_error(void);       /* thread-local, static storage */
/* MEAN_SIZE_ARR (tools/static_model.py:17-21) as the library holds it: 9 floats, (3 size clusters) x (l, w, h), HOST
 * memory with static storage. The one copy that the decode and criterion kernels are compiled with; a binding that
 * keeps the table on its side as well (3dal_pytorch_amd/arch.py) compares the two when it loads the library. */
const float* dal3_mean_size(void);

/* Fold BN (eps 1e-5) into each layer and write the MFMA-fragment-ordered / row-major image the
 * kernels consume. Call with packed_dev == NULL to query *bytes_inout. Layers come in forward
 * order (ins_seg: conv1..5, dconv1..5; *_BOX_EST / *_EMB: conv1..4 then fc1..).
 * Replaces: nothing in the reference (it keeps nn.Conv1d/nn.BatchNorm1d modules,
 * static_model.py:249-269); this is the derived cache of SURVEY.md 8(b).
 * The image is opaque and its size may change between builds of the library: always take it from the query. The
 * DAL3_F32 image of DAL3_HEAD_INS_SEG ends (in front of its tail padding) with the compacted dconv2's region: the
 * folded dconv2 weights once more, [k 0..511 in the kernel's accumulation order][row 0..31][out-tile 0..7] fp32
 * (512 KiB), and a 256-byte section whose first int32 is nonzero when a folded dconv2 weight is not finite or a folded
 * dconv2 bias is -0: the decode kernel then never skips a dead channel (DESIGN.md "Compacted dconv2"). */
int dal3_pack_weights(int head_kind, const dal3_layer* layers, int n_layers, int dtype,
                      void* packed_dev, size_t* bytes_inout, dal3_stream stream);

/* logical (B, C, N) tensor with element strides: the callers hand pts.transpose(2,1) of a
 * point-major buffer, i.e. strides (N*C, 1, C) (static_eval.py:265); contiguous (C*N, N, 1)
 * is accepted too. dtype = how the values are STORED: DAL3_F32 (0, what a zero-initialised struct says), DAL3_BF16 or
 * DAL3_F16 — 16-bit points / box windows (BASELINE.json configs C3, C5: "bf16 storage") are read in place and widened
 * exactly in the kernels' loads, no fp32 copy is made; `data` then points at 2-byte elements and the strides count
 * those. Independent of the arithmetic dtype of the packed weights. Outputs are fp32 whatever the storage. */
typedef struct {
    const float* data;
    int64_t stride_b, stride_c, stride_n;
    int32_t dtype;
    int32_t flags;                       /* MUST be 0 or a mask of DAL3_BCN_* (was `reserved` before 0.1.3: a caller that never
                                          * zeroed it now gets DAL3_EINVAL for unknown bits, or a different — bit-identical
                                          * — kernel family for bits 1 / 2 / 4; zero-initialise the struct) */
} dal3_bcn;

/* Per-call dispatch hints (dal3_bcn.flags; dal3_static_args / dal3_dynamic_args take them from args.pts.flags for every
 * kernel of the call). Which kernel family runs is a function of the job's size and of these bits ONLY — the library
 * reads no environment variable and keeps no process-wide switch. Results are bit-identical either way; the bits exist
 * for A/B measurements and for the tests that pin that identity (tests/test_gpu_latency.py, test_gpu_parity.py).
 *   DAL3_BCN_NO_SMALL_JOB_KERNELS  never the small-job ("latency") family (jobs of <= 512 tiles of 32 points)
 *   DAL3_BCN_NO_WORKLIST           point heads: one workgroup per (item, tile) instead of the live-tile worklist
 *   DAL3_BCN_NO_LDS_SAMPLER        mask compaction + sampling: positions through global memory, keys recomputed per
 *                                  pass (what items of more than 7936 points always take) instead of both in LDS
 *   DAL3_BCN_NO_DEC_PLAN           fp32 instance segmentation: the decoder computes every dconv1 channel of every tile
 *                                  instead of leaving out the channels that the encoder's bound proves dead for the whole
 *                                  crop (large jobs only; 8 is not a flag and stays refused)
 *   DAL3_BCN_NO_ENC_RESIDENT       fp32 instance segmentation: the screened encoder as its two launches (bound, then
 *                                  candidates; four workgroups per 1024 points) instead of one workgroup per crop, which
 *                                  jobs of many crops take (dal3_ins_seg_encoder_route)
 *   DAL3_BCN_NO_HEAD_RESIDENT      fp32 static box_est / point_emb heads: the screened conv4 as its two launches (dense
 *                                  seed tiles, then the other tiles) instead of one workgroup per item, which jobs of
 *                                  many items take (dal3_point_head_route)
 *   DAL3_BCN_NO_DEC_PAIR           fp32 instance segmentation: the throughput decoder with one wave per 32-point tile
 *                                  instead of a pair of waves per tile (dal3_ins_seg_decode_route) */
enum { DAL3_BCN_NO_SMALL_JOB_KERNELS = 1, DAL3_BCN_NO_WORKLIST = 2, DAL3_BCN_NO_LDS_SAMPLER = 4, DAL3_BCN_NO_DEC_PLAN = 16,
       DAL3_BCN_NO_ENC_RESIDENT = 32, DAL3_BCN_NO_HEAD_RESIDENT = 64, DAL3_BCN_NO_DEC_PAIR = 128 };

/* ---- PointNetInstanceSeg.forward (static_model.py:271-296, dynamic_model.py:187-212) plus
 * the mask of point_cloud_masking (static_model.py:59). logits (B,N,2) fp32, mask (B,N) u8.
 * workspace: dal3_ins_seg_workspace_bytes(B). global_feat_out optional (B,1024). */
size_t dal3_ins_seg_workspace_bytes(int B);
/* Where a DAL3_F32 dal3_ins_seg_forward of a large job (the screened encoder and the throughput decoder both run, and
 * DAL3_BCN_NO_DEC_PLAN is not set) leaves the decoder's plan in its workspace, as byte offsets: off[0] (B,513) u32, per
 * crop the order-preserving keys of the maxima U_c of dconv1's fp16 scores (natural channel order; key = bits ^ 0x80000000
 * for a non-negative value, ~bits for a negative one, 0 = nothing seen) and in word 512 the fp32 bits of X = max ||x2||_2
 * (+Inf: no bound); off[1] (B,640) u32, the unflagged chain indices (k = 32 c + 2 r + h for channel 32 c + (r & 3) +
 * 8 (r >> 2) + 4 h) in ascending order, padded with 512, the null channel; off[2] (B,512) f32, the crop's dconv1 term
 * gathered to match (-1 for the null channel); off[3] (B) i32, the chunk count (even; 0 = fewer than *min_dead channels
 * are flagged and the decoder runs as without a plan). For tests and measurements. */
int dal3_ins_seg_plan_layout(int B, size_t off[4], int* min_dead);
/* Which encoder a DAL3_F32 instance-segmentation job of B crops x N points takes with `flags` (DAL3_BCN_*) on the current
 * device: the small-job family, the dense throughput kernel (short jobs), the screened encoder's two launches, or its
 * crop-resident single launch. A pure function of its arguments and the device's CU count; negative (DAL3_EINVAL) for a
 * bad argument. For tests and measurements: results are bit-identical on every route. */
enum { DAL3_ENC_ROUTE_LATENCY = 0, DAL3_ENC_ROUTE_DENSE = 1, DAL3_ENC_ROUTE_TWO_LAUNCH = 2, DAL3_ENC_ROUTE_RESIDENT = 3 };
int dal3_ins_seg_encoder_route(int B, int N, int flags);
/* Which decoder a DAL3_F32 instance-segmentation job of B crops x N points takes with `flags` on the blob `packed`: the
 * small-job family, the throughput kernel with one wave per tile, or the one with a pair of waves per tile. A blob whose
 * guard flag is set (a folded dconv2 - dconv4 weight is not finite, or a folded bias is -0) never takes the pairs. The
 * flag is in device memory: this call reads it with a blocking copy (packed == NULL: taken as clear); the launch itself
 * decides on the device. Negative (DAL3_EINVAL) for a bad argument. For tests and measurements: the same bits on every route. */
enum { DAL3_DEC_ROUTE_LATENCY = 0, DAL3_DEC_ROUTE_ONE_WAVE = 1, DAL3_DEC_ROUTE_PAIR = 2 };
int dal3_ins_seg_decode_route(const void* packed, int B, int N, int flags);
int dal3_ins_seg_forward(const void* packed, int dtype, int c_in, dal3_bcn pts, int B, int N,
                         float* logits, uint8_t* mask, float* global_feat_out,
                         void* workspace, size_t workspace_bytes, dal3_stream stream);

/* The three kernels of dal3_ins_seg_forward as separate launches (per-kernel timing and tests):
 *   encode      conv1..conv5 + BN + ReLU with the max over N fused (static_model.py:279-284):
 *               pts -> global_feat (B,1024); global_feat must be zero-filled by the caller
 *   global_bias the per-crop part of dconv1 (its 1024 global-feature columns, :286-289):
 *               global_feat -> gbias (B,512) = W1g' g + b1'
 *   decode      dconv1 (64 per-point columns) .. dconv5 + mask (:289-295, :59) */
int dal3_ins_seg_encode(const void* packed, int dtype, int c_in, dal3_bcn pts, int B, int N, float* global_feat,
                        dal3_stream stream);
int dal3_ins_seg_global_bias(const void* packed, int dtype, const float* global_feat, int B, float* gbias,
                             dal3_stream stream);
int dal3_ins_seg_decode(const void* packed, int dtype, int c_in, dal3_bcn pts, int B, int N, const float* gbias,
                        float* logits, uint8_t* mask, dal3_stream stream);

/* ---- gather_object_pts (static_model.py:23-49 / dynamic_model.py:24-50) on the device.
 * counts (B) i32 = number of segmented points; obj_idx (B,M) i32 = chosen point indices;
 * obj_pts (B,M,C) fp32 point-major = pts[:, :C, idx] (all-zero rows where count == 0, as the
 * reference leaves them). choice: see DAL3_SAMPLER_CHOICE (NULL for DAL3_SAMPLER_DEVICE).
 * item_offset = global index of item 0 (multi-GPU shards draw the same subset as one GPU).
 * workspace: dal3_gather_workspace_bytes(B, N). */
size_t dal3_gather_workspace_bytes(int B, int N);
int dal3_segment_counts(const uint8_t* mask, int B, int N, int32_t* counts, dal3_stream stream);
int dal3_mask_compact_sample(const uint8_t* mask, dal3_bcn pts, int B, int N, int C, int M,
                             int sampler, const int32_t* choice, uint64_t seed, int64_t item_offset,
                             int32_t* counts, int32_t* obj_idx, float* obj_pts,
                             void* workspace, size_t workspace_bytes, dal3_stream stream);

/* The device sampler with its draw counter in DEVICE memory: key = (seed, *step, global item index, rank). Training
 * draws fresh object points every step (the reference's np.random stream moves on, static_model.py:36-47); a step
 * captured into a hipGraph must not freeze that, so the counter is a device scalar the caller bumps with a captured op
 * (step == NULL: as dal3_mask_compact_sample with DAL3_SAMPLER_DEVICE). */
int dal3_mask_compact_sample_step(const uint8_t* mask, dal3_bcn pts, int B, int N, int C, int M, uint64_t seed,
                                  const int64_t* step, int64_t item_offset, int32_t* counts, int32_t* obj_idx,
                                  float* obj_pts, void* workspace, size_t workspace_bytes, dal3_stream stream);

/* ---- shared MLP (4 x Conv1d k=1 + BN + ReLU) + channel-wise max over the point axis + the FC
 * stack of the head: static PointNetEstimation.forward (static_model.py:320-339) -> (B,39);
 * PointEmbedding.forward (dynamic_model.py:234-249) -> (B,256); BoxEmbedding.forward
 * (:271-286) -> (B,128). out has row stride out_stride floats (so the two embeddings can be
 * written side by side: the torch.cat of dynamic_model.py:137).
 * workspace: dal3_point_head_workspace_bytes(B). */
size_t dal3_point_head_workspace_bytes(int B);
int dal3_point_head_forward(int head_kind, const void* packed, int dtype, dal3_bcn x, int B, int M,
                            float* out, int64_t out_stride,
                            void* workspace, size_t workspace_bytes, dal3_stream stream);

/* The per-point stack + max of the same heads as its own launch (conv1..4 + BN + ReLU, torch.max(x, 2)[0]:
 * static_model.py:329-334, dynamic_model.py:240-245, :277-282) -> feat (B,512), no FC tail; per-kernel timing and
 * tests. n_distinct (B) i32 device or NULL: only the first n_distinct[b] points of item b differ, the others repeat
 * one of them (what dal3_mask_compact_sample's device sampler writes when fewer than M points are segmented);
 * repeated points cannot change a max over points, so the kernel skips them. The whole-model sequencers pass
 * `counts` here. */
/* workspace (optional): dal3_point_head_pool_workspace_bytes(B, M) bytes of 16-byte aligned device scratch for the
 * list of tiles that hold distinct points; with it large jobs run as persistent waves over that list instead of one
 * workgroup per (item, tile) — same bits either way. NULL / too small: the per-tile launch. */
size_t dal3_point_head_pool_workspace_bytes(int B, int M);
int dal3_point_head_pool(int head_kind, const void* packed, int dtype, dal3_bcn x, int B, int M,
                         const int32_t* n_distinct, float* feat, void* workspace, size_t workspace_bytes,
                         dal3_stream stream);
/* How the fp32 static box_est / point_emb heads take their screened route (conv4 on the fp16 MFMA, candidates
 * recomputed exactly: same bits): with a workspace, from this many 32-point tiles (B * ceil(M / 32)) upward; every
 * `stride`-th live tile of an item is its dense seed. Dispatch facts for tests and measurements. */
int dal3_point_head_screen_min_tiles(void);
int dal3_point_head_screen_stride(void);
/* Which kernels a DAL3_F32 point-head job of B items x M points takes with `flags` (DAL3_BCN_*) on the current device, a
 * workspace given: the small-job family, one workgroup per (item, tile), the dense persistent waves, the screened conv4's
 * two launches, or its item-resident single launch. A pure function of its arguments and the device's CU count; negative
 * (DAL3_EINVAL) for a bad argument. For tests and measurements: results are bit-identical on every route. */
enum { DAL3_HEAD_ROUTE_LATENCY = 0, DAL3_HEAD_ROUTE_PER_TILE = 1, DAL3_HEAD_ROUTE_PERSISTENT = 2, DAL3_HEAD_ROUTE_TWO_LAUNCH = 3,
       DAL3_HEAD_ROUTE_RESIDENT = 4 };
int dal3_point_head_route(int head_kind, int B, int M, int flags);

/* ---- dynamic PointNetEstimation.forward (dynamic_model.py:300-312): (B,384) -> (B,39). */
int dal3_dynamic_box_est_forward(const void* packed, const float* embedding, int B, float* box_pred,
                                 void* workspace, size_t workspace_bytes, dal3_stream stream);

/* ---- parse_output_to_tensors (static_model.py:64-96) + the eval drivers' box decode
 * (static_eval.py:269-288, dynamic_eval.py:226-242, utils.py:69-79).
 * box_pred (B,39) -> heading_residuals (B,12), size_residuals (B,9), center (B,3), boxes7 (B,7)
 * [cx,cy,cz,l,w,h,yaw]. center = box_pred[:, :3] + center_add[:, :3] (center_add may be NULL),
 * written back into box_pred[:, :3] too when center_inplace != 0 (the reference's
 * `center_one += init_box[:, :3]` mutates box_pred through a view, static_model.py:174).
 * boxes7 centre = center (+ boxes_center_add[:, :3] when not NULL: the dynamic driver adds
 * init_box[:, :3] only at decode time). yaw = class2angle(argmax) + yaw_base[b*yaw_stride]. */
int dal3_decode_boxes(float* box_pred, int B,
                      const float* center_add, int64_t center_add_stride, int center_inplace,
                      const float* boxes_center_add, int64_t boxes_center_add_stride,
                      const float* yaw_base, int64_t yaw_stride,
                      float* heading_residuals, float* size_residuals, float* center, float* boxes7,
                      dal3_stream stream);

/* ---- the re-centring between the two box estimators of StaticModelTwoBoxEst
 * (static_model.py:192-205, rotz :98-106): p <- Rz(-yaw_one) (Rz(yaw_init) p + c_init - c_one),
 * plus the stage-two heading labels angle2class(bbox_gt[:, -1] - box_one[:, -1], 12)
 * (utils.py:53-60). obj_pts/obj_pts_two (B,M,3) point-major. bbox_gt may be NULL. */
int dal3_recenter_rotz(const float* obj_pts, int B, int M, const float* init_box7,
                       const float* box_one7, const float* bbox_gt7, float* obj_pts_two,
                       int64_t* heading_class_label, float* heading_residual_label,
                       dal3_stream stream);

/* ---- torch.max(x, 2)[0] as a standalone kernel (static_model.py:284,334): x (B,C,N)
 * contiguous fp32 -> out (B,C). The HBM-roofline kernel of BASELINE.json. */
int dal3_maxpool_n(const float* x, int64_t rows, int64_t n, float* out, dal3_stream stream);
/* The same for rows stored as DAL3_F32, DAL3_BF16 or DAL3_F16 (BASELINE.json configs C3 / C5: "bf16 storage"; 2-byte rows
 * move half the bytes: B*C*N*2 + B*C*2): x (rows, n) contiguous in `dtype`, out (rows) in the same dtype. Exact — the
 * maximum is one of the inputs — and, as torch.max, NaN for a row that holds a NaN (both entries). */
int dal3_maxpool_n_dtype(const void* x, int dtype, int64_t rows, int64_t n, void* out, dal3_stream stream);

/* ---- crop preparation right before the heads, float64 in, fp32 out ------------------
 * STATICTRACK.__getitem__ (static_model.py:529-546, 568-572) for B tracks at once: points = all frames' points
 * of every track stacked, global frame, (P_total,3) f64; offsets (B+1) delimit the tracks; pose (B,16) =
 * inv(veh_to_global) of each track's best-score frame, row-major; box (B,7) f64 = that frame's detection
 * already moved to the vehicle frame (transform_box, :574-588; a per-track scalar job the host does).
 * pts_out (B,N,3) fp32 point-major = Rz(-yaw)(pose p - centre) of N points drawn WITH replacement: choice
 * (B,N) i32 holds the draws (np.random.choice(P_b, N) for bit-reproducing the reference) or is NULL for the
 * device RNG keyed on (seed, item_offset + b, n). init_box_out (B,7) fp32 = box. */
int dal3_static_crop_prep(const double* points, const int64_t* offsets, const int32_t* choice,
                          const double* pose, const double* box, int B, int N, uint64_t seed,
                          int64_t item_offset, float* pts_out, float* init_box_out, dal3_stream stream);

/* DYNAMICTRACK.__getitem__ (dynamic_model.py:429-453, 490-507) for B items: per-frame point arrays of all
 * tracks concatenated (points (P_total,3) f64, frame_offsets (F_total+1)), per-frame global boxes (F_total,7)
 * f64, track_first (n_tracks+1) = first frame of each track in those arrays; item b = frame item_frame[b] of
 * track item_track[b]; pose (B,16) = inv(veh_to_global) of that frame. Outputs: pts_out (B,(2r+1)*n_per,4) with
 * the 0.1*(j-r) time channel, box_out (B,2s+1,8) with 0.1*(j-s), init_box_out (B,8) (the centre box before
 * re-centring). The reference's quirks are kept: missing/empty frames give zero points that are still moved by
 * the pose and the re-centring; missing boxes are zero rows that are still pose-transformed; points are rotated
 * by -yaw of the centre box, boxes only translated (yaw made relative). choice (B,2r+1,n_per) i32 or NULL. */
int dal3_dynamic_item_prep(const double* points, const int64_t* frame_offsets, const double* boxes,
                           const int64_t* track_first, const int32_t* item_track, const int32_t* item_frame,
                           const int32_t* choice, const double* pose, int B, int n_per, int r, int s,
                           uint64_t seed, int64_t item_offset, float* pts_out, float* box_out,
                           float* init_box_out, dal3_stream stream);

/* ---- write-back of refined boxes into the per-frame detections: the det_annos update of
 * postprocessing() in static_eval.py:71-87,148-155 and dynamic_eval.py:53-64,121-129, for P (track, frame) pairs.
 * final_boxes (n,7) f64, final_idx (P): which refined box a pair carries; pose_best (P,16) f64 veh_to_global of the
 * track's best frame (static) or NULL (dynamic: the box already is in the pair's frame); pose_inv (P,16) f64
 * inv(veh_to_global) of the pair's frame; track_box (P,7) f64 the track's own global box in that frame (the search
 * key); det (n_det,7) fp32 all frames' detections concatenated, UPDATED IN PLACE; det_start/det_count (P): the
 * pair's frame in det; active (P) u8: the reference skips frames that lack the matched GT object.
 * match (P) i32 out: matched row within the frame or -1; owner (n_det) i32 scratch. When two pairs hit one row
 * the later pair wins, as in the reference's sequential loop. */
int dal3_writeback_boxes(const double* final_boxes, const int32_t* final_idx, const double* pose_best,
                         const double* pose_inv, const double* track_box, float* det, const int64_t* det_start,
                         const int32_t* det_count, const uint8_t* active, int P, int64_t n_det, int32_t* match,
                         int32_t* owner, dal3_stream stream);

/* ---- the mask labels of the prepared items (training side of SURVEY.md 8(f) N1): static_model.py:548-556,
 * dynamic_model.py:455-487. Same inputs and the same draws (choice, or seed/item_offset) as the *_prep calls
 * above, so label n belongs to output point n. Face equations: (.,6,4) f64 rows [nx,ny,nz,d] of the matched
 * annotation's box as det3d's surface_equ_3d_jitv2 gives them (geometry.py:351-377) — O(#boxes) host work with
 * NumPy, see dal3_points_in_boxes. mask_label u8 in {0,1}.
 * static: gt_planes (B,6,4); the test runs on the vehicle-frame point `pose p` (before re-centring).
 * dynamic: window frame j of item b is tested in frame j's own vehicle frame: q = xform[b][j] (pose p) with
 * xform (B,2r+1,16) = inv(veh_to_global_j) @ inv(pose_b) (dynamic_model.py:481), planes (B,2r+1,6,4),
 * valid (B,2r+1) u8 = frame j has the matched annotation; out-of-track or invalid frames give zeros. */
int dal3_static_crop_labels(const double* points, const int64_t* offsets, const int32_t* choice, const double* pose,
                            int B, int N, uint64_t seed, int64_t item_offset, const double* gt_planes,
                            uint8_t* mask_label, dal3_stream stream);
int dal3_dynamic_item_labels(const double* points, const int64_t* frame_offsets, const int64_t* track_first,
                             const int32_t* item_track, const int32_t* item_frame, const int32_t* choice,
                             const double* pose, int B, int n_per, int r, uint64_t seed, int64_t item_offset,
                             const double* xform, const double* planes, const uint8_t* valid, uint8_t* mask_label,
                             dal3_stream stream);

/* ---- points-in-rotated-box: det3d box_np_ops.points_in_rbbox (det3d/core/bbox/box_np_ops.py:641-647 ->
 * geometry.py:240-275) as a (P,K) u8 table. points: P rows of >= 3 values, `stride` values apart, float32
 * (points_f64 = 0) or float64; planes (K,6,4) f64. A point is outside as soon as ((x nx + y ny) + z nz) + d >= 0
 * for a face, each operation rounded on its own; evaluated in float32 when f32_math != 0 (float32 points AND
 * float32 boxes, the reference's sweep case), in float64 otherwise. NaN coordinates count as inside (as there). */
int dal3_points_in_boxes(const void* points, int points_f64, int64_t P, int64_t stride, const double* planes, int K,
                         int f32_math, uint8_t* inside, dal3_stream stream);

/* ---- rotated-box IoU: the quantity of det3d/ops/iou3d_nms/iou3d_nms_utils.py boxes_iou_bev / boxes_iou3d_gpu.
 * Boxes (.,7) row-major [x, y, z, l, w, h, yaw] (z the centre, yaw about +z, l along the heading: the det3d convention
 * boxes_iou3d_gpu takes before its to_pcdet mirror, and the one the heads emit), float32 (boxes_f64 = 0) or float64
 * (boxes_f64 = 1). Outputs are float32; iou_bev and iou_3d may each be NULL (that output is skipped), not both.
 *   iou_bev = area(A n B) / area(A u B) of the bird's-eye-view rectangles;
 *   iou_3d  = area(A n B) * z_overlap / (l_a w_a h_a + l_b w_b h_b - area(A n B) * z_overlap)   (iou3d_nms_utils.py:52-72).
 * A union <= 0 gives 0, a non-finite input NaN for its pairs, a negative size counts as 0. The centre and yaw
 * differences of a pair are taken in the input precision, the rest in float32: the result does not depend on where
 * the pair sits in the world. dal3_box_iou_pairwise(a[i], b[j]) and dal3_box_iou_paired on that pair are the same bits.
 * Bounds: n, m <= DAL3_MAX_ITEMS and the launch grid (ceil(n/16) * ceil(m/64), resp. ceil(n/256)) <= DAL3_MAX_TILES. */
int dal3_box_iou_pairwise(const void* a, int64_t n, const void* b, int64_t m, int boxes_f64, float* iou_bev,
                          float* iou_3d, dal3_stream stream);   /* (n, m) row-major */
int dal3_box_iou_paired(const void* a, const void* b, int64_t n, int boxes_f64, float* iou_bev, float* iou_3d,
                        dal3_stream stream);                    /* (n): a[k] vs b[k] */

/* ---- box-estimation training metrics: compute_box3d_iou (tools/utils.py:81-103) plus the per-epoch accumulation of
 * static_train.py:96-129 / static_eval.py:204-250 for one batch of B items, in ONE launch, with no host sync.
 * Per item, on both sides (prediction / label), in float64:
 *   heading = hc (2 pi / 12) + residual[hc], minus 2 pi when > pi          (class2angle(..., to_label_format=True))
 *   size    = MEAN_SIZE[sc] + size_residual[sc]                            (class2size)
 * with hc = argmax(heading_scores[0:12]), sc = argmax(size_scores[0:3]) on the prediction side (first index on ties,
 * a NaN is the maximum: np.argmax / torch.argmax) and the class labels on the label side; then the BEV and 3D IoU of
 * the pair [center, size, heading] through the function of dal3_box_iou_paired with float64 boxes: iou_bev[k] and
 * iou_3d[k] are the bits of dal3_box_iou_paired(pred_k, label_k, boxes_f64 = 1). A class label outside its range gives
 * NaN for that item (nothing is read out of the row). Segmentation: correct = argmax(logits[b, n, 0:2]) ==
 * (int64)mask_label[b, n], torch.argmax's rule; a non-finite float mask label never matches.
 *
 * Every per-item field is read through its row stride (in elements); the elements of a row are contiguous (a (B,3,3)
 * size_residuals row is its 9 values). Float fields are float32 unless their DAL3_BM_* bit is set in f64_fields;
 * class labels are int64 unless their bit is set in i32_fields.
 *
 * Accumulation (acc, may be NULL when an output is given and logits is NULL): stream-ordered read-modify-write, so a
 * run of calls on one stream sums batch after batch. The float sums of a batch are formed by one workgroup in a
 * fixed order and the counts are integers: the accumulator is bitwise reproducible run to run. No workspace. */
enum { DAL3_BM_CENTER = 1, DAL3_BM_HEADING_SCORES = 2, DAL3_BM_HEADING_RESIDUALS = 4, DAL3_BM_SIZE_SCORES = 8,
       DAL3_BM_SIZE_RESIDUALS = 16, DAL3_BM_CENTER_LABEL = 32, DAL3_BM_HEADING_RESIDUAL_LABEL = 64,
       DAL3_BM_SIZE_RESIDUAL_LABEL = 128 };                            /* f64_fields */
enum { DAL3_BM_HEADING_CLASS_LABEL = 1, DAL3_BM_SIZE_CLASS_LABEL = 2 };  /* i32_fields */
enum { DAL3_MASK_U8 = 0, DAL3_MASK_F32 = 1 };                           /* mask_dtype: uint8 / bool, float32 */

typedef struct dal3_box_metric_acc {     /* 48 bytes; zero it to start an epoch */
    double sum_iou_bev;                  /* sum of iou_bev over the items */
    double sum_iou_3d;                   /* sum of iou_3d */
    double sum_loss;                     /* sum of *loss over the calls that gave one */
    uint64_t n_iou_3d_pass;              /* items with iou_3d >= thr (float32 compare; NaN does not pass) */
    uint64_t n_seg_correct;              /* points whose argmax matches the mask label */
    uint64_t n_items;                    /* items (B per call) */
} dal3_box_metric_acc;

typedef struct dal3_box_metric_args {
    int64_t B, N;                        /* items; points per item (segmentation term) */
    const void* center;                  int64_t ld_center;                  /* (B,3) */
    const void* heading_scores;          int64_t ld_heading_scores;          /* (B,12) */
    const void* heading_residuals;       int64_t ld_heading_residuals;       /* (B,12) */
    const void* size_scores;             int64_t ld_size_scores;             /* (B,3) */
    const void* size_residuals;          int64_t ld_size_residuals;          /* (B,3,3) */
    const void* center_label;            int64_t ld_center_label;            /* (B,3) */
    const void* heading_class_label;     int64_t ld_heading_class_label;     /* (B) */
    const void* heading_residual_label;  int64_t ld_heading_residual_label;  /* (B) */
    const void* size_class_label;        int64_t ld_size_class_label;        /* (B) */
    const void* size_residual_label;     int64_t ld_size_residual_label;     /* (B,3) */
    int32_t f64_fields;                  /* DAL3_BM_* bits */
    int32_t i32_fields;                  /* DAL3_BM_*_CLASS_LABEL bits */
    const float* logits;                 /* (B,N,2) float32 at the strides below; NULL: no segmentation term */
    int64_t logits_stride_b, logits_stride_n, logits_stride_c;
    const void* mask_label;              /* (B,N) at the strides below, mask_dtype */
    int64_t mask_stride_b, mask_stride_n;
    int32_t mask_dtype;
    float thr;                           /* the box estimation accuracy threshold on iou_3d */
    const float* loss;                   /* optional: one float32 value added to acc->sum_loss (in float64) */
    float* iou_bev;                      /* optional (B) float32 */
    float* iou_3d;                       /* optional (B) float32 */
    dal3_box_metric_acc* acc;            /* optional, see above */
} dal3_box_metric_args;

/* Bounds: B <= DAL3_MAX_ITEMS, N <= DAL3_MAX_POINTS_PER_ITEM, 1 + B ceil(N / 1024) <= DAL3_MAX_TILES. */
int dal3_box_estimation_metrics(const dal3_box_metric_args* args, dal3_stream stream);

/* ---- tracking run: CenterPoint's greedy tracker (tools/waymo_tracking/tracker.py, PubTracker.step_centertrack, driven
 * by test.py:84-134) over every frame of S sequences in ONE call, and the ground-truth match of
 * _create_pd_detection(tracking=True) (det3d/datasets/waymo/waymo_common.py:173-189).
 *
 * dal3_track: frames are flat, sequence after sequence, in the order test.py's sort_detections gives them
 * (seq_id * 1000 + frame_id); sequence s = frames [seq_offsets[s], seq_offsets[s+1]), its first frame the
 * `frame_id == 0` frame that resets the tracks (the id counter runs on); frame f = detections
 * [frame_offsets[f], frame_offsets[f+1]), numbered within the frame as box ids. Per detection: ct (K,2) float64 global
 * x, y; tracking (K,2) float64 = velocity * -1 * time_lag; label 0..2; score float32. The detection side of the
 * distance is float32(ct + float32(tracking)), the track side float32(ct); every tracker.py rule is kept bit for bit
 * (dal3_track.hip restates each with its line). Output: frame f's active entries (tracker.py `active != 0`: matched,
 * then new) at [frame_offsets[f], frame_offsets[f] + out_count[f]): box_ids (the detection's index in its frame) and
 * tracking_ids (int64, counted from *id_base + 1 — id_base optional, NULL = 0 — across the sequences in order, as the
 * reference's one tracker counts them). id_total (optional) = *id_base + the ids handed out: pass it as the next
 * call's id_base to continue the count on the device.
 * capacity: live tracks per sequence, <= DAL3_TRACK_MAX_CAPACITY. With max_age A, a frame never holds more than the
 * detections of its last A frames (a track of age a came from a detection a - 1 frames back), so that sum's maximum
 * over the sequence is always enough. A sequence that needs more sets DAL3_TRACK_OVERFLOW in *status (ids then
 * undefined); a label outside 0..2 sets DAL3_TRACK_BAD_LABEL (that detection matches nothing). status is OR-ed
 * into, zero it first. max_workgroups (0: one per sequence) caps the grid; the result does not depend on it.
 * workspace: dal3_track_workspace_bytes(S, K, capacity). */
#define DAL3_TRACK_MAX_CAPACITY 65536
enum { DAL3_TRACK_OVERFLOW = 1, DAL3_TRACK_BAD_LABEL = 2, DAL3_TRACK_BAD_ID = 4 };   /* status bits */

typedef struct dal3_track_args {
    int64_t S, F, K;                     /* sequences, frames, detections */
    const int64_t* seq_offsets;          /* (S+1) into the frames */
    const int64_t* frame_offsets;        /* (F+1) into the detections */
    const double* ct;                    /* (K,2) */
    const double* tracking;              /* (K,2) */
    const int32_t* label;                /* (K) */
    const float* score;                  /* (K) */
    float max_dist[3];                   /* max_diff per class: VEHICLE, PEDESTRIAN, CYCLIST (float32 compare) */
    int32_t max_age;
    double score_thresh;                 /* a new id needs score > score_thresh (float64 compare) */
    int64_t capacity;
    int32_t max_workgroups;
    int32_t reserved;
    const int64_t* id_base;              /* optional (1) */
    int32_t* box_ids;                    /* (K) */
    int64_t* tracking_ids;               /* (K) */
    int32_t* out_count;                  /* (F) */
    int64_t* id_total;                   /* optional (1) */
    int32_t* status;                     /* (1) */
    void* workspace;
    size_t workspace_bytes;
} dal3_track_args;

/* dal3_track_match: for every output entry of dal3_track (frame order, then output order) the 3D IoU of its box
 * against its frame's annotation boxes (dal3_box_iou_* geometry, float32 boxes, the detection as `a`): boxes (K,7)
 * Waymo convention [x,y,z,l,w,h,heading] by detection (row frame_offsets[f] + box id); gt_boxes (G,7) =
 * obj['box'][[0,1,2,3,4,5,-1]], frame f's at [gt_offsets[f], gt_offsets[f+1]). The first maximum counts; a NaN in the
 * row or a maximum not above thr gives none. A tracking id's match is its first candidate in that order, kept for every
 * later entry of the id (`matching`); entries before it have none. Out: match_frame / match_obj (K) by output position,
 * -1 for None. Ids must lie in (*id_base, *id_base + K] (else DAL3_TRACK_BAD_ID). workspace:
 * dal3_track_match_workspace_bytes(K). */
typedef struct dal3_track_match_args {
    int64_t F, K;
    const int64_t* frame_offsets;        /* (F+1) as for dal3_track */
    const int32_t* out_count;            /* (F) */
    const int32_t* box_ids;              /* (K) */
    const int64_t* tracking_ids;         /* (K) */
    const int64_t* id_base;              /* optional (1), as given to dal3_track */
    const float* boxes;                  /* (K,7) */
    const int64_t* gt_offsets;           /* (F+1) */
    const float* gt_boxes;               /* (G,7) */
    float thr;                           /* 0.75 */
    int32_t reserved;
    int32_t* match_frame;                /* (K) */
    int32_t* match_obj;                  /* (K) */
    int32_t* status;                     /* (1) */
    void* workspace;
    size_t workspace_bytes;
} dal3_track_match_args;

size_t dal3_track_workspace_bytes(int64_t S, int64_t K, int64_t capacity);
int dal3_track(const dal3_track_args* args, dal3_stream stream);
size_t dal3_track_match_workspace_bytes(int64_t K);
int dal3_track_match(const dal3_track_match_args* args, dal3_stream stream);

/* ---- motion-state run: the regrouping of tools/trackData.py as a stable sort on the device, trackFeature of
 * tools/motionState.py:30-67, the GT table of tools/trackGT.py:43-66 and the decision of SVC(kernel='linear').
 * Every entry below is enqueued on `stream` and reads nothing back; problems are OR-ed into a device status word
 * (DAL3_MOTION_BAD_KEY shares the word and the numbering of the DAL3_TRACK_* bits).
 *
 * dal3_group_by_key: a stable counting sort of E entries by key = keys[i] - (*key_base, optional) - key_bias into
 * T groups: group g's entries are entry[group_start[g] : group_start[g + 1]], input positions in ascending order
 * (= frame order, the order trackData.py appends in). With frame_offsets / out_count (both or neither; as dal3_track
 * holds them) only slots frame_offsets[f] + [0, out_count[f]) are entries. group_start[T] = the number of entries
 * grouped; n_groups (optional) = the largest key + 1. T is the caller's capacity (E always suffices for ids counted
 * from 1). A key outside [0, T) sets DAL3_MOTION_BAD_KEY and the entry is left out. The result is a function of the
 * input alone: the same bits for every max_workgroups (0 = no cap) and every run.
 * E, T <= DAL3_MAX_ITEMS. workspace: dal3_group_workspace_bytes(E, T). */
enum { DAL3_MOTION_BAD_KEY = 8 };                /* status bit, beside DAL3_TRACK_* */

typedef struct dal3_group_args {
    int64_t E, T, F;                     /* entries (slots), group capacity, frames (0 without frame_offsets) */
    const int64_t* keys;                 /* (E) */
    const int64_t* key_base;             /* optional (1), subtracted on the device (dal3_track's id_base) */
    int64_t key_bias;                    /* subtracted too: 1 for tracking ids, which are counted from id_base + 1 */
    const int64_t* frame_offsets;        /* optional (F+1) */
    const int32_t* out_count;            /* optional (F) */
    int64_t* group_start;                /* (T+1) */
    int32_t* entry;                      /* (E) */
    int64_t* n_groups;                   /* optional (1) */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;              /* 0: no cap */
    void* workspace;
    size_t workspace_bytes;
} dal3_group_args;

/* dal3_track_features: per group of a dal3_group_by_key result, over per-entry arrays indexed by input position:
 * n, type[first], match[last], sum(n_points), best = position inside the group of the first maximum of score
 * (np.argmax), keep = !(match[last] < 0 || n < 7 || type[first] == 2 || sum(n_points) == 0), and
 * feature = [ ||c[first] - c[last]||, ||var(c, axis=0)|| ] in float64: the mean is the sequential sum in entry order
 * / n, the variance the sequential sum of squared deviations / n (NumPy's two passes; an empty group gives zeros). */
typedef struct dal3_track_feature_args {
    int64_t T, E;
    const int64_t* group_start;          /* (T+1) */
    const int32_t* entry;                /* (E) */
    const int64_t* n_groups;             /* optional (1): dal3_group_by_key's; groups from there on are empty */
    const double* center;                /* (E,3) global frame */
    const int32_t* type;                 /* (E) */
    const float* score;                  /* (E) */
    const int32_t* n_points;             /* (E) */
    const int32_t* match;                /* (E) GT object index or -1 */
    int32_t* n;                          /* (T) */
    int32_t* type0;                      /* (T) */
    int32_t* match_last;                 /* (T) */
    int64_t* points_sum;                 /* (T) */
    int32_t* best;                       /* (T) */
    uint8_t* keep;                       /* (T) */
    double* feature;                     /* (T,2) */
    int64_t max_workgroups;
} dal3_track_feature_args;

/* dal3_gt_table: entries are annotation rows: box (E,9) float64 = obj['box'] in its frame's vehicle frame, frame (E)
 * the row's frame, pose (F,16) that frame's veh_to_global. Per entry box_global (E,7) = transform_box of
 * box[[0,1,2,3,4,5,8]] and vel = ||box[6:8]||; per group (GT object) n, dist = ||c[first] - c[last]||, max_vel and
 * is_static = dist < 1 && max_vel < 1. A frame index outside [0, F) sets DAL3_MOTION_BAD_KEY (that row becomes NaN). */
typedef struct dal3_gt_table_args {
    int64_t T, E, F;
    const int64_t* group_start;          /* (T+1) */
    const int32_t* entry;                /* (E) */
    const double* box;                   /* (E,9) */
    const int32_t* frame;                /* (E) */
    const double* pose;                  /* (F,16) */
    double* box_global;                  /* (E,7) */
    double* vel;                         /* (E) */
    int32_t* n;                          /* (T) */
    double* dist;                        /* (T) */
    double* max_vel;                     /* (T) */
    uint8_t* is_static;                  /* (T) */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;
} dal3_gt_table_args;

/* dal3_motion_classify: decision = feature[0] * w[0] + feature[1] * w[1] + b (float64, in that order), is_static =
 * decision > 0 for every group; the kept groups are compacted in ascending group order into static_ids and
 * dynamic_ids, counts = {statics, dynamics}. workspace: dal3_motion_classify_workspace_bytes(T). */
typedef struct dal3_motion_classify_args {
    int64_t T;
    const double* feature;               /* (T,2) */
    const uint8_t* keep;                 /* (T) */
    double w[2];
    double b;
    double* decision;                    /* (T) */
    uint8_t* is_static;                  /* (T) */
    int32_t* static_ids;                 /* (T) */
    int32_t* dynamic_ids;                /* (T) */
    int64_t* counts;                     /* (2) */
    int64_t max_workgroups;
    void* workspace;
    size_t workspace_bytes;
} dal3_motion_classify_args;

size_t dal3_group_workspace_bytes(int64_t E, int64_t T);
int dal3_group_by_key(const dal3_group_args* args, dal3_stream stream);
int dal3_track_features(const dal3_track_feature_args* args, dal3_stream stream);
int dal3_gt_table(const dal3_gt_table_args* args, dal3_stream stream);
size_t dal3_motion_classify_workspace_bytes(int64_t T);
int dal3_motion_classify(const dal3_motion_classify_args* args, dal3_stream stream);

/* ---- baseline runs: the tracker's own boxes scored against ground truth — the per-(track, frame) loop of
 * tools/static_init.py:58-141 (calculate_init_iou), :143-241 (calculate_static_iou) and tools/dynamic_init.py:37-123,
 * and the "best IoU over the frame's GT boxes" of tools/eval.py:72-87. (Additions only; DAL3_VERSION is pinned by the
 * existing tests, as for dal3_track.)
 *
 * dal3_score_tracks: S samples = (track, frame) pairs from flat tables. Per sample s, in float64:
 *   init   = transform_box(boxes[box_row[s]], pose_inv[frame[s]]): centre = (R c summed in einsum's order) + t,
 *            yaw + atan2(R10, R00)                                                  (static_init.py:42-56)
 *   pred   = [init centre, class2size(size2class(init size)), 0.0]   (class2angle(angle2class(0)) is exactly 0.0)
 *   label  = [gt centre (NOT rotated into init's frame: the reference's quirk, kept), class2size(size2class(gt size)),
 *             class2angle(angle2class(gt yaw - init yaw))]                          (tools/utils.py:53-79)
 * and the pair goes through the function of dal3_box_iou_paired with float64 boxes: iou_bev[s] / iou_3d[s] are the bits
 * of dal3_box_iou_paired(pred_s, label_s, boxes_f64 = 1). "Own box" is box_row[s] = the sample's own row, "best box"
 * box_row[s] = the row of its track's best-score frame: one kernel. pose_inv is inv(veh_to_global) formed by the caller
 * (np.linalg.inv on the host). gt (S,7) = obj['box'][[0,1,2,3,4,5,-1]] of the matched object, float32 (gt_f64 = 0, the
 * annotations' dtype) or float64, read only where has_gt[s] != 0. A sample without ground truth — or whose box_row /
 * frame lies outside [0, R) / [0, F), which is the caller's contract — is NOT scored: NaN in every per-sample output,
 * nothing added to the sums, but counted in n_samples (static_init.py:71,157: the means divide by all samples).
 * Accuracy: iou_3d >= thr[0] / thr[1] / thr[2] for type 1 / 2 / 4, thr_other for any other type (float32 compare; NaN
 * does not pass); the static / dynamic scripts differ only in these numbers and in how they read n_type.
 *
 * Accumulation (acc optional when an output is given): the sums ADD into *acc, stream-ordered, so the calls of a
 * split's track files accumulate without a host read. Reproducible: sample s belongs to chunk s / 256 whatever the
 * grid; a chunk is reduced in a fixed tree and written to the workspace with ordinary stores, and a second
 * one-workgroup launch adds the chunks in a fixed order. The accumulator's bytes are a function of the inputs and the
 * order of the calls alone (not of max_workgroups, not of the scheduling); no floating-point atomics. The float64 sums
 * are of the float32 per-sample values (NumPy of the reference's time; today's accumulates them in float32).
 * workspace: dal3_score_workspace_bytes(S), needed only with acc; contents undefined afterwards.
 * Bounds: S, R, F <= DAL3_MAX_ITEMS. S == 0 succeeds and launches nothing (acc is left as it is). */
typedef struct dal3_score_acc {          /* 72 bytes; zero it to start a run */
    double sum_iou_bev;                  /* sum of iou_bev over the scored samples */
    double sum_iou_3d;                   /* sum of iou_3d */
    uint64_t n_iou_3d_pass;              /* scored samples at or above their type's threshold */
    uint64_t n_type[4];                  /* scored samples of type 1, 2, 4, any other */
    uint64_t n_scored;                   /* samples with ground truth */
    uint64_t n_samples;                  /* all samples (S per call): the means' denominator */
} dal3_score_acc;

typedef struct dal3_score_args {
    int64_t S, R, F;                     /* samples, box rows, frames */
    const double* boxes;                 /* (R,7) global-frame track boxes [x,y,z,l,w,h,yaw] */
    const int32_t* box_row;              /* (S) row of `boxes` the sample is scored with */
    const int32_t* frame;                /* (S) row of pose_inv */
    const double* pose_inv;              /* (F,16) row-major inv(veh_to_global) */
    const void* gt;                      /* (S,7) float32, or float64 when gt_f64 != 0 */
    const uint8_t* has_gt;               /* (S) */
    const int32_t* type;                 /* (S) Waymo type of the track-frame */
    int32_t gt_f64;                      /* 0 or 1 */
    int32_t max_workgroups;              /* 0: 8 per CU of the current device; the result does not depend on it */
    float thr[3];                        /* iou_3d threshold of type 1, 2, 4 */
    float thr_other;                     /* ... of any other type */
    float* iou_bev;                      /* optional (S) */
    float* iou_3d;                       /* optional (S) */
    double* pred_box;                    /* optional (S,7): the decoded prediction; NULL = not written */
    double* label_box;                   /* optional (S,7): the decoded label */
    dal3_score_acc* acc;                 /* optional, see above */
    void* workspace;
    size_t workspace_bytes;
} dal3_score_args;

size_t dal3_score_workspace_bytes(int64_t S);
int dal3_score_tracks(const dal3_score_args* args, dal3_stream stream);

/* dal3_best_gt_iou: Q query boxes, query q against the GT boxes [gt_offsets[f], gt_offsets[f+1]) of its own frame
 * f = query_frame[q] (tools/eval.py:72-87: boxes_iou3d_gpu of a (1,7) box against the frame's (G,7), np.max /
 * np.argmax). Boxes float32 (boxes_f64 = 0, what eval.py casts to) or float64, both sides alike. best_iou_3d[q] = the
 * maximum of dal3_box_iou_pairwise(query, gt)'s 3D IoU over the range (the same bits), best_iou_bev[q] the BEV IoU of
 * that pair, best_index[q] the FIRST arg-max within the range (a NaN counts as the maximum, as np.argmax has it). An
 * empty range, or a frame outside [0, F), gives NaN and -1. Ranges are clipped to [0, G]. Q, F <= DAL3_MAX_ITEMS.
 * Q == 0 succeeds and launches nothing. No workspace. */
typedef struct dal3_best_gt_args {
    int64_t Q, F, G;                     /* queries, frames, GT boxes */
    const void* queries;                 /* (Q,7) */
    const int32_t* query_frame;          /* (Q) */
    const int64_t* gt_offsets;           /* (F+1) into gt_boxes */
    const void* gt_boxes;                /* (G,7) */
    int32_t boxes_f64;                   /* 0 or 1 */
    int32_t max_workgroups;              /* 0: 8 per CU of the current device */
    float* best_iou_3d;                  /* (Q) */
    float* best_iou_bev;                 /* optional (Q) */
    int32_t* best_index;                 /* optional (Q) */
} dal3_best_gt_args;

int dal3_best_gt_iou(const dal3_best_gt_args* args, dal3_stream stream);

/* ---- detector post-processing: the non-maximum suppression of det3d/core/bbox/box_torch_ops.py:248-277
 * (rotate_nms_pcdet -> iou3d_nms_cuda.nms_gpu, det3d/ops/iou3d_nms/iou3d_nms_utils.py:75-92) and of
 * det3d/core/utils/circle_nms_jit.py (center_head.py:498-506), for F segments in one enqueue with no host round trip,
 * and the head decode of det3d/models/bbox_heads/center_head.py:342-419, 459-471.
 *
 * dal3_nms. A segment is one (frame, task) pair: rows [seg_offsets[f], seg_offsets[f+1]) of boxes (K, box_stride) and
 * scores (K) float32, of which the first n = seg_count[f] are used (seg_count optional: NULL = all of them). Boxes are
 * [x, y, z, l, w, h, ...] in the det3d convention with the yaw in column yaw_col (6 for plain (K,7) boxes; 8 with
 * box_stride 9 reads center_head.py:471's boxes_for_nms out of the 9-column boxes without a copy), float32 or float64.
 * The boxes are taken as dal3_box_iou_pairwise takes them (column 3 the extent along the yaw): what nms_gpu is handed.
 * rotate_nms_pcdet first converts ITS boxes to that convention (box_torch_ops.py:255-257: columns 3 and 4 swapped,
 * yaw -> -yaw - pi/2). The centres stay while the rectangles turn from yaw to -yaw, so this is not an isometry of the
 * pair and it does change the IoUs; mirror = 1 applies it as each box is loaded, in the input precision (float32:
 * -yaw - float32(pi/2), as torch forms it), and every statement below then holds for the converted boxes.
 * Per segment the result is defined exactly:
 *   order       the rows by score descending, NaN scores first (torch.sort(descending=True), argsort()[::-1]), equal
 *               scores (-0 == +0) by ascending row. The reference's sorts are not stable; this order is the definition here.
 *   candidates  the first m = min(n, pre_max) of that order (pre_max 0: no cut), m <= DAL3_NMS_MAX_PRE.
 *   scan        in that order a candidate is kept when no earlier KEPT candidate suppresses it. DAL3_NMS_ROTATE: i
 *               suppresses j when iou_bev(i, j) > thresh, iou_bev the bits of dal3_box_iou_pairwise(box_i, box_j); a NaN
 *               IoU suppresses nothing (a non-finite box is kept and suppresses nobody). DAL3_NMS_CIRCLE: i suppresses j
 *               when dx*dx + dy*dy <= thresh, dx and dy the centre differences (taken in the input precision, rounded
 *               to float32), the two products and the sum each rounded in float32; the SQUARED distance is compared
 *               with thresh as given, as circle_nms does.
 *   output      the kept candidates' rows relative to the segment, in scan order, the first post_max of them
 *               (post_max 0: no cut): keep[f * stride + [0, keep_count[f])). The scan stops at post_max keeps.
 * stride >= min(post_max or N, N), N the largest segment (by seg_offsets). seg_offsets is given twice: on the device for
 * the kernels and on the HOST (seg_offsets_host, the same values, read only during the call) for the checks made before
 * any launch: non-decreasing, within [0, K], stride. order (optional, (K)): the full sorted order of every segment at
 * its rows. Nothing is read back: a segment whose candidates exceed DAL3_NMS_MAX_PRE (pre_max 0 and n larger) sets
 * DAL3_NMS_TOO_MANY in *status and keeps nothing; device offsets that differ from a valid CSR set DAL3_NMS_BAD_SEGMENT
 * likewise. status is OR-ed into (the bits are numbered beside DAL3_TRACK_* / DAL3_MOTION_*). The result is a function
 * of the segment alone: the same for every max_workgroups (0: one workgroup per segment), every run, and however the
 * segments are split over calls. Only the IoUs of KEPT candidates against later ones are ever evaluated and no n x n
 * mask exists: workspace is dal3_nms_workspace_bytes(K, boxes_f64) = O(K). F, K <= DAL3_MAX_ITEMS. */
#define DAL3_NMS_MAX_PRE 65536
enum { DAL3_NMS_ROTATE = 0, DAL3_NMS_CIRCLE = 1 };
enum { DAL3_NMS_TOO_MANY = 16, DAL3_NMS_BAD_SEGMENT = 32, DAL3_DECODE_OVERFLOW = 64 };   /* status bits */

typedef struct dal3_nms_args {
    int64_t F, K;                        /* segments, rows */
    const int64_t* seg_offsets;          /* (F+1) device */
    const int64_t* seg_offsets_host;     /* (F+1) HOST copy of the same values */
    const int32_t* seg_count;            /* optional (F) device: rows in use per segment (dal3_center_decode's) */
    const void* boxes;                   /* (K, box_stride) */
    const float* scores;                 /* (K) */
    int64_t box_stride;                  /* elements per box row, >= 7 */
    int32_t yaw_col;                     /* 6 <= yaw_col < box_stride */
    int32_t boxes_f64;                   /* 0 or 1 */
    int32_t mode;                        /* DAL3_NMS_ROTATE / DAL3_NMS_CIRCLE */
    float thresh;
    int64_t pre_max, post_max;           /* 0: no cut */
    int64_t stride;                      /* keep's row length */
    int32_t max_workgroups;              /* 0: one per segment */
    int32_t mirror;                      /* 0 or 1: convert each box as rotate_nms_pcdet does (see above) */
    int32_t* keep;                       /* (F, stride) */
    int32_t* keep_count;                 /* (F) */
    int32_t* order;                      /* optional (K) */
    int32_t* status;                     /* (1) OR-ed */
    void* workspace;
    size_t workspace_bytes;
} dal3_nms_args;

size_t dal3_nms_workspace_bytes(int64_t K, int boxes_f64);
int dal3_nms(const dal3_nms_args* args, dal3_stream stream);

/* dal3_center_decode: CenterHead.predict's arithmetic for one task (center_head.py:342-419; with double_flip:
 * dal3_center_decode_flip4 below) and post_processing's masks (center_head.py:459-469), B samples in one enqueue. The
 * maps are float32 views (B, H, W, C) with ELEMENT strides: NHWC as the reference's permute(0, 2, 3, 1).contiguous()
 * leaves them, or the network's NCHW as it is. Per cell (row, col), every operation a separately rounded float32, in this order:
 *   score = max over classes of sigmoid(hm) = 1 / (1 + exp(-hm)), label = the FIRST maximum (torch.max);
 *   x = ((col + reg[0]) * out_size_factor) * voxel_size[0] + pc_range[0], y likewise from row and reg[1]; z = height;
 *   dim = exp(dim); rot = atan2(rot[0], rot[1]).
 * A cell survives when score > score_threshold (a NaN fails) and, with has_range, x, y, z lie inside
 * post_center_limit_range = range[0..2] .. range[3..5] inclusive. Sample b's survivors go, IN CELL ORDER (an ordered
 * compaction by ballot scans: no atomic decides a position), to the rows of segment f = seg_first + b * seg_step:
 * boxes (K, 9) [x, y, z, dim0, dim1, dim2, vel0, vel1, rot] with vel, else (K, 7); scores; labels (class within the
 * task); cell = row * W + col; seg_count[f] = their number. A segment holds seg_offsets[f+1] - seg_offsets[f] rows:
 * more survivors set DAL3_DECODE_OVERFLOW in *status and the first that fit are kept; nothing is written outside the
 * segment's rows, nor outside [0, K) (DAL3_NMS_BAD_SEGMENT). H * W <= DAL3_MAX_ITEMS, B <= DAL3_MAX_ITEMS, C <= 64.
 * workspace: dal3_center_decode_workspace_bytes(B, H, W). */
typedef struct dal3_map {
    const float* data;
    int64_t stride_b, stride_h, stride_w, stride_c;   /* in elements */
} dal3_map;

typedef struct dal3_center_decode_args {
    int64_t B, H, W;
    int32_t C;                           /* classes of this task (hm's channels) */
    int32_t has_range;                   /* 0: post_center_limit_range is empty */
    dal3_map hm, reg, height, dim, rot, vel;   /* vel.data NULL: no velocity, 7-column boxes */
    float out_size_factor;
    float voxel_size[2];
    float pc_range[2];
    float score_threshold;
    float range[6];
    int64_t F, K;                        /* segments and rows of the outputs */
    int64_t seg_first, seg_step;         /* sample b -> segment seg_first + b * seg_step */
    const int64_t* seg_offsets;          /* (F+1) device */
    float* boxes;                        /* (K, 9 or 7) */
    float* scores;                       /* (K) */
    int32_t* labels;                     /* (K) */
    int32_t* cell;                       /* (K) */
    int32_t* seg_count;                  /* (F): written for this call's segments only */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;              /* 0: no cap */
    void* workspace;
    size_t workspace_bytes;
} dal3_center_decode_args;

size_t dal3_center_decode_workspace_bytes(int64_t B, int64_t H, int64_t W);
int dal3_center_decode(const dal3_center_decode_args* args, dal3_stream stream);

/* dal3_center_decode_flip4: CenterHead.predict with test_cfg.double_flip (center_head.py:318-414) for one task: the
 * un-flip of the four views' maps, their merge and the decode above in one pass, no intermediate map written.
 * decode.B is the number of MERGED samples; every map holds 4 * decode.B samples, sample b's view v at map index
 * 4 b + v in the order Reformat returns them (formating.py:78): v = 0 the sweep as it is, 1 with y = -y, 2 with x = -x,
 * 3 with both. Output cell (row, col) reads view v at
 *   v = 0: (row, col)   v = 1: (H-1-row, col)   v = 2: (row, W-1-col)   v = 3: (H-1-row, W-1-col),
 * and with a_v the value there and mean(a0, a1, a2, a3) = (((a0 + a1) + a2) + a3) / 4, every operation a separately
 * rounded float32 in exactly this order (torch.mean(dim=1) on a CPU tensor):
 *   score_k = mean over v of sigmoid(hm_v[k]) (the mean of the sigmoids); score = the max over k, label = the FIRST
 *             maximum, a NaN wins and stays;
 *   reg_x   = mean(r0, r1, 1 - r2, 1 - r3) of reg[0], reg_y = mean(r0, 1 - r1, r2, 1 - r3) of reg[1]; x and y from
 *             col + reg_x and row + reg_y as dal3_center_decode forms them;
 *   z       = mean of height; dim_j = mean of exp(dim_v[j]);
 *   rot     = atan2(mean(s0, s1, -s2, -s3), mean(c0, -c1, c2, -c3)), s = rot[0], c = rot[1];
 *   vel     = (mean(vx0, vx1, -vx2, -vx3), mean(vy0, -vy1, vy2, -vy3)).
 * The score and range masks, the ordered compaction, boxes / scores / labels / cell / seg_count of segment
 * seg_first + b * seg_step, the status bits and every bound are dal3_center_decode's, with B the merged samples.
 * workspace: dal3_center_decode_flip4_workspace_bytes(B, H, W) (B merged samples). */
typedef struct dal3_center_decode_flip4_args {
    dal3_center_decode_args decode;      /* B: MERGED samples; the maps hold 4 B */
} dal3_center_decode_flip4_args;

size_t dal3_center_decode_flip4_workspace_bytes(int64_t B, int64_t H, int64_t W);
int dal3_center_decode_flip4(const dal3_center_decode_flip4_args* args, dal3_stream stream);

/* dal3_flip4_points: DoubleFlip's three copies (det3d/datasets/pipelines/test_aug.py) of B samples' points, laid out
 * as the batch of 4 B samples the detector then runs on. points (N, C) float32 contiguous, C >= 2; sample b is rows
 * [offsets[b], offsets[b+1]) (device, non-decreasing within [0, N]). out (4 N, C): sample b's four views are consecutive,
 * view v at rows [out_offsets[4 b + v], out_offsets[4 b + v + 1]) with out_offsets[4 b + v] = 4 offsets[b] + v n_b,
 * n_b the sample's rows, out_offsets[4 B] = 4 offsets[B]; each view holds the sample's rows in their order with column 1
 * negated for v = 1, column 0 for v = 2, both for v = 3. The negation flips the sign bit (0.0 -> -0.0, a NaN keeps its
 * payload: NumPy's unary minus); columns >= 2 are copied. One enqueue, every input element read once, nothing read
 * back; a row that device offsets would send outside out is not written. B == 0 succeeds with nothing launched.
 * B, N <= DAL3_MAX_ITEMS / 4. */
int dal3_flip4_points(const float* points, int64_t N, int32_t C, const int64_t* offsets, int64_t B, float* out,
                      int64_t* out_offsets, int64_t max_workgroups, dal3_stream stream);

/* dal3_sweep_merge: the WaymoDataset branch of LoadPointCloudFromFile (det3d/datasets/pipelines/loading.py:61-91,
 * 140-168) for B samples in one enqueue. A sample is nsweeps (1 .. DAL3_SWEEP_MAX) segments, the current frame first and
 * then info["sweeps"][0 .. nsweeps - 2] in that order; the table `segments` (DEVICE memory, B * nsweeps entries, sample b's
 * at [b nsweeps, (b + 1) nsweeps)) names each one's raw rows where they lie, xyz (n, 3) and feature (n, 2) float32 in planes
 * of their own (the frame file's lidars.points_xyz / points_feature, uploaded as they are). out (N, C) float32 contiguous,
 * C = 5 for nsweeps == 1 and 6 otherwise: segment s fills rows [out_row, out_row + n) with
 *     [x', y', z', tanh(feature0), feature1 (, time)]
 * where (x', y', z') = (x, y, z) bit for bit without a transform, and with one the first three rows of
 * matrix (3 x 4 row-major, float64) . [x, y, z, 1]: ((m0 x + m1 y) + m2 z) + m3 in float64, every product and sum rounded
 * on its own, cast to float32 once. tanh is the float64 tanh of the float32 value cast once (1e5 gives exactly 1.0f); NaN
 * and infinities go through as IEEE-754 has them. time is the segment's, 0 for a current frame. The segments' out_row
 * must ascend and partition [0, N) in table order (out_row[s + 1] = out_row[s] + n[s]); a row that a table sends nowhere
 * is not written, and no row outside out ever is. point_offsets (B + 1) int64, device, is written: point_offsets[b] =
 * the out_row of sample b's current frame, point_offsets[B] = N. Every output element is written once by one lane: no
 * atomic, the same bits for every max_workgroups (0: no cap). B == 0 succeeds with nothing launched.
 * B * nsweeps <= DAL3_MAX_ITEMS, N <= DAL3_MAX_TILES. */
#define DAL3_SWEEP_MAX 16
typedef struct dal3_sweep_segment {
    const float* xyz;                    /* (n, 3) device */
    const float* feature;                /* (n, 2) device */
    int64_t n;
    int64_t out_row;
    double matrix[12];                   /* the first three rows of transform_matrix; read only with has_transform */
    float time;                          /* float32(time_lag); 0 for the current frame */
    int32_t has_transform;               /* 0: transform_matrix is None, or the current frame */
} dal3_sweep_segment;

int dal3_sweep_merge(const dal3_sweep_segment* segments, int64_t B, int32_t nsweeps, int64_t N, float* out,
                     int64_t* point_offsets, int64_t max_workgroups, dal3_stream stream);

/* ---- the PointPillars reader: points_to_voxel (det3d/ops/point_cloud/point_cloud_ops.py:7-184, through
 * VoxelGenerator.generate and collate_kitti's batch column), PillarFeatureNet and PointPillarsScatter
 * (det3d/models/readers/pillar_encoder.py:15-209) and VoxelFeatureExtractorV3 (voxel_encoder.py:9-24), for B samples in
 * one enqueue with no host round trip.
 *
 * dal3_voxelize. points (N, point_stride) float32, the first C (3 <= C <= 8) columns of a row are the point; sample b is
 * rows [point_offsets[b], point_offsets[b+1]) (given on the device and, the same values, on the HOST for the checks made
 * before any launch). Defined exactly, per sample:
 *   cell        c_j = floor((p_j - pc_range[j]) / voxel_size[j]), j = x, y, z: a float32 subtraction, a correctly rounded
 *               float32 division, a floor. The point is dropped when c_j < 0 or c_j >= grid[j] for any j (a lower face
 *               is in, an upper face is out; +-Inf fails the test as in the reference) or p_j is NaN (the reference casts
 *               the NaN to an index, which is undefined). grid = round((hi - lo) / size) in float32 comes from the caller.
 *   voxel       a cell's voxel index is its rank by first appearance among the sample's in-range points in input order;
 *               cells of rank >= max_voxels are dropped with all their points, later points of an earlier cell are kept.
 *   rows        the voxel's first max_points points in input order, all C columns, zeros after them;
 *               num_points = min(count, max_points).
 *   coordinates [b, z, y, x] with reverse_index (what VoxelGenerator asks for), else [b, x, y, z], int32.
 * The samples' voxels are packed back to back: sample b's are rows [voxel_offsets[b], voxel_offsets[b+1]) of voxels
 * (capacity, max_points, C), coordinates (capacity, 4) and num_points (capacity); voxel_offsets (B+1) is written on the
 * device. capacity >= the sum over samples of min(points of the sample, max_voxels, cells of the grid), which the host
 * knows; rows from voxel_offsets[B] on are zero. No atomic decides a position: a stable least-significant-digit radix
 * sort of (sample, cell) keys over chunks of 4096 points (histogram, scan, scatter, as dal3_group_by_key) orders the
 * points of a cell by their index, the head of each run is flagged at its original position, an exclusive scan of the
 * flags in point order is the voxel index and a point's place in its run is its row. The result is a function of the
 * input alone, the same for every max_workgroups and every run, and of a sample alone whatever else is in the batch.
 * Device offsets that differ from the host's so that a row would fall outside the capacity set DAL3_PILLAR_OVERFLOW in
 * *status (OR-ed) and the row is not written. B * cells < 2^31 - 1, N <= DAL3_MAX_ITEMS, max_points <= 64 * 1024.
 * workspace: dal3_voxelize_workspace_bytes(B, N) = O(N). */
enum { DAL3_PILLAR_OVERFLOW = 128 };     /* status bit, numbered beside DAL3_NMS_* */

typedef struct dal3_voxelize_args {
    int64_t B, N;                        /* samples, rows of points */
    const float* points;                 /* (N, point_stride) */
    int64_t point_stride;                /* elements per row, >= C */
    int32_t C;                           /* 3 .. 8 */
    int32_t reverse_index;               /* 0 or 1 */
    const int64_t* point_offsets;        /* (B+1) device */
    const int64_t* point_offsets_host;   /* (B+1) HOST copy of the same values */
    float voxel_size[3];
    float pc_range[6];
    int32_t grid[3];                     /* cells along x, y, z */
    int32_t max_points;
    int64_t max_voxels;                  /* per sample */
    int64_t capacity;                    /* rows of the outputs */
    float* voxels;                       /* (capacity, max_points, C) */
    int32_t* coordinates;                /* (capacity, 4) */
    int32_t* num_points;                 /* (capacity) */
    int64_t* voxel_offsets;              /* (B+1) */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;              /* 0: no cap */
    void* workspace;
    size_t workspace_bytes;
} dal3_voxelize_args;

size_t dal3_voxelize_workspace_bytes(int64_t B, int64_t N);
int dal3_voxelize(const dal3_voxelize_args* args, dal3_stream stream);

/* dal3_pillar_pack: the eval-mode PFNLayers (Linear without bias, BatchNorm1d, ReLU) of a PillarFeatureNet folded, in
 * float64 and rounded once, to W' = W * g / sqrt(var + eps), b' = beta - mean * g / sqrt(var + eps), and laid out as the
 * MFMA fragments the feature kernel keeps in registers. layers: 1 (C + 5 -> 64) or 2 (C + 5 -> 32, 64 -> 64), every
 * pointer of a layer but `bias` (which must be NULL) a device pointer. out: DAL3_PILLAR_PACK_FLOATS floats.
 *
 * dal3_pillar_features: (voxels, num_points, coordinates) -> features (P, c_out) in one kernel. Per pillar, in float32,
 * each operation rounded by itself (no contraction where a product feeds a sum):
 *   mean        the sum over all max_points rows (padding rows are zero) / num_points;
 *   row         [p (C columns), p_xyz - mean, x - (coor_x * vx + x_offset), y - (coor_y * vy + y_offset)], times the
 *               padding mask (row < num_points); coor_x = coordinates[3], coor_y = coordinates[2] (the reversed layout);
 *   layer 1     relu(W1' row + b1') for EVERY one of the max_points rows (a padding row carries relu(b1')), the max over them;
 *   layer 2     relu(W2a' x + (W2b' max1 + b2')) for every row, W2' = [W2a' | W2b'], the max over the rows.
 * The products run on the fp32 MFMA with channels on its rows and the pillar's rows on its columns; columns beyond
 * max_points repeat a real row and never take part as zeros. With `canvas` the result goes to canvas[b, :, y, x] of a
 * (canvas_B, c_out, ny, nx) map that the call first fills with +0, and `features` may be NULL; without it the rows go to
 * features. n_pillars (optional, device): only the first min(*n_pillars, P) pillars exist (voxel_offsets[B] of
 * dal3_voxelize). A pillar whose coordinates fall outside the canvas is not written. 1 <= max_points <= 64.
 *
 * dal3_pillar_scatter: features (P, c_out) -> the same canvas, zero-filled first; cells are unique per sample, so no
 * atomics. dal3_voxel_mean: VoxelFeatureExtractorV3, out (P, C) = the sum over the max_points rows / num_points. */
#define DAL3_PILLAR_PACK_FLOATS 5120

typedef struct dal3_pillar_feature_args {
    int64_t P;                           /* rows of voxels / features */
    const int64_t* n_pillars;            /* optional device (1): pillars in use */
    const float* voxels;                 /* (P, max_points, C) */
    const int32_t* num_points;           /* (P) */
    const int32_t* coordinates;          /* (P, 4) [b, z, y, x] */
    int32_t C, max_points;
    int32_t n_layers, c_out;             /* 1 or 2; 64 */
    float vx, vy, x_offset, y_offset;
    const float* packed;                 /* dal3_pillar_pack's */
    float* features;                     /* (P, c_out), or NULL with a canvas */
    float* canvas;                       /* optional (canvas_B, c_out, ny, nx) */
    int64_t canvas_B, ny, nx;
    int64_t max_workgroups;              /* 0: no cap */
} dal3_pillar_feature_args;

int dal3_pillar_pack(const dal3_layer* layers, int n_layers, int C, double eps, float* out, dal3_stream stream);
int dal3_pillar_features(const dal3_pillar_feature_args* args, dal3_stream stream);
int dal3_pillar_scatter(const float* features, const int32_t* coordinates, int64_t P, const int64_t* n_pillars, int c_out,
                        float* canvas, int64_t canvas_B, int64_t ny, int64_t nx, dal3_stream stream);
int dal3_voxel_mean(const float* voxels, const int32_t* num_points, int64_t P, const int64_t* n_pillars, int max_points, int C,
                    float* out, dal3_stream stream);

/* ---- the reader's training step: PFNLayer in train mode (det3d/models/readers/pillar_encoder.py:40-55), forward and
 * backward, on the rows dal3_pillar_features defines above (the same mean, decoration and padding mask), float32 inputs,
 * products on the fp32 MFMA, every sum over pillars in float64.
 *
 * Live pillars. live = min(*n_pillars, P) with n_pillars, else P; the BatchNorm sees n = live * max_points samples.
 * Nothing of a pillar behind `live` is read, counted or written: its voxels and num_points may hold anything, NaN included.
 * Forward, per layer, x the layer's input row:
 *   z = W x (no bias); mean_c and var_c (biased) over all n rows. PADDING ROWS COUNT: their layer-1 z is exactly 0, so they
 *   add nothing to the sums but are part of n. xhat = (z - mean) / sqrt(var + eps), a = gamma xhat + beta (evaluated as one
 *   fused multiply-add z * (gamma istd) + (beta - mean gamma istd)), y = relu(a); top = the max of y over all max_points
 *   rows, padding rows included. A middle layer passes on [y | top repeated], the last layer passes on top.
 *   Shapes: units [64] or [32, 64], 3 <= C <= 8, 1 <= max_points <= 64, one eps.
 * Running statistics (optional: running_mean[l] NULL leaves layer l's alone), on the device, in float64, rounded once:
 *   r = (1 - momentum) r + momentum * stat, the variance unbiased: var * n / max(n - 1, 1); num_batches_tracked += 1.
 *   live == 0 gives mean 0 and var 0.
 * Backward, from the cotangent of the last layer's top:
 *   da = dy [a > 0]; dbeta = sum da, dgamma = sum da xhat; dz = gamma / sqrt(var + eps) (da - dbeta / n - xhat dgamma / n)
 *   for EVERY row of every live pillar: a padding row has a non-zero dz and, in layer 2, the non-zero input
 *   [y1_pad | top1], so it contributes to dW2 and to what flows back into layer 1. dW = sum over rows dz (x) x,
 *   dx = W^T dz. The max sends its cotangent to the lowest row that attains it; a middle layer's top receives the sum
 *   of its repeated columns' dx over the pillar's rows. Rows that tie exactly are at y = 0 (the ReLU gate stops the
 *   cotangent) or have identical inputs (the same terms whichever is picked): the choice shows in no parameter gradient.
 *   No gradient with respect to the voxels is produced.
 * Sums. Every sum over pillars (sum z, sum z^2, dbeta, dgamma, dW) is taken over slices of DAL3_PILLAR_TRAIN_SLICE
 * consecutive pillars, in pillar order, into float64; every slice's partial is stored and the partials are added in
 * ascending slice order, in float64. No floating-point atomic: the bits are the same for every max_workgroups and every
 * run. MFMA columns beyond max_points (a repeated row) are masked out of every sum. Nothing of P * max_points * channels
 * elements is written to memory. Nothing synchronises.
 * Outputs. forward: `features` (P, 64), first filled with +0 (rows behind live stay 0), or, with `canvas`, the
 * (canvas_B, 64, ny, nx) map of dal3_pillar_features (zero-filled first; a pillar outside the canvas is not written), and
 * `saved`, DAL3_PILLAR_TRAIN_SAVED_FLOATS floats, 16-byte aligned: per layer mean | istd | gamma istd | beta - mean gamma
 * istd, 64 each. backward: the same geometry, parameters and `saved`; `grad` is the cotangent of features (element strides
 * grad_stride[0] per row, [1] per channel) or, when `canvas` is non-NULL (only its being set is used), of the canvas with
 * strides grad_stride[0..3] per (b, c, y, x): a channels-last or sliced cotangent is read as it lies, a pillar outside
 * the canvas has a zero cotangent. dW[l] (units, c_in), dgamma[l], dbeta[l] (units) are written, not added to.
 * layers: a HOST array of n_layers dal3_layer with device pointers weight, bn_weight, bn_bias (bias NULL; bn_mean, bn_var unused).
 * workspace: dal3_pillar_train_workspace_bytes(P, n_layers), 8-byte aligned; the backward does not need the forward's. */
#define DAL3_PILLAR_TRAIN_SLICE 128
#define DAL3_PILLAR_TRAIN_SAVED_FLOATS 512

typedef struct dal3_pillar_train_args {
    int64_t P;                           /* rows of voxels / features */
    const int64_t* n_pillars;            /* optional device (1): pillars in use */
    const float* voxels;                 /* (P, max_points, C) */
    const int32_t* num_points;           /* (P) */
    const int32_t* coordinates;          /* (P, 4) [b, z, y, x] */
    int32_t C, max_points;
    int32_t n_layers, c_out;             /* 1 or 2; 64 */
    float vx, vy, x_offset, y_offset;
    const dal3_layer* layers;            /* HOST (n_layers) */
    double eps;
    double momentum[2];
    float* running_mean[2];              /* forward: optional, per layer (units) */
    float* running_var[2];
    int64_t* num_batches_tracked[2];     /* forward: optional, per layer (1) */
    float* saved;                        /* (DAL3_PILLAR_TRAIN_SAVED_FLOATS): forward writes, backward reads */
    float* features;                     /* forward: (P, c_out), or NULL with a canvas */
    float* canvas;                       /* optional (canvas_B, c_out, ny, nx); backward: non-NULL selects the canvas cotangent */
    int64_t canvas_B, ny, nx;
    const float* grad;                   /* backward: the cotangent */
    int64_t grad_stride[4];              /* elements: (row, channel, -, -) or (b, c, y, x) */
    float* dW[2];                        /* backward outputs, per layer */
    float* dgamma[2];
    float* dbeta[2];
    int64_t max_workgroups;              /* 0: no cap */
    void* workspace;
    size_t workspace_bytes;
} dal3_pillar_train_args;

size_t dal3_pillar_train_workspace_bytes(int64_t P, int n_layers);
int dal3_pillar_train_forward(const dal3_pillar_train_args* args, dal3_stream stream);
int dal3_pillar_train_backward(const dal3_pillar_train_args* args, dal3_stream stream);

/* ---- the detector's dense stage: the 2-D convolutions of RPN (det3d/models/necks/rpn.py) and of CenterHead.forward /
 * SepHead (det3d/models/bbox_heads/center_head.py:65-110, 167-244), float32, eval mode.
 *
 * The fold. dal3_conv2d_pack, dal3_sp_conv_pack and dal3_roi_pack fold a layer's optional eval-mode BatchNorm into its
 * weight and bias by ONE rule (csrc/dal3_fold.h), with the layer's own eps, in float64, every operation rounded by
 * itself (no fused multiply-add), in this order, and one rounding of W' and b' to float32:
 *   scale = g / sqrt(var + eps)      the sum, the square root, the quotient
 *   W'    = W * scale
 *   b'    = ((bias - mean) * scale) + beta
 * Without BatchNorm scale = 1 and b' = bias; a NULL bias is 0. A BatchNorm needs all four of weight, bias, mean and var
 * and an eps > 0; out is 16-byte aligned.
 *
 * A layer is Conv + optional BatchNorm2d + optional ReLU with the BatchNorm folded by dal3_conv2d_pack (the fold above;
 * the neck's norm_cfg says eps 1e-3, the head's nn.BatchNorm2d 1e-5). Three forms, x and y float32 NCHW
 * tensors read and written through the element strides of a dal3_map, a (B, H, W, C) view:
 *   DAL3_CONV2D_3X3      y[b,co,oy,ox] = act(b'[co] + sum W'[co,ci,ky,kx] * x[b,ci,oy*s+ky-1,ox*s+kx-1]), zeros outside the
 *                        image, s = stride 1 or 2, output (floor((H-1)/s)+1, floor((W-1)/s)+1): both ZeroPad2d(1) +
 *                        Conv2d(3, stride=s) and Conv2d(3, padding=1). weight (c_out, c_in, 3, 3).
 *   DAL3_CONV2D_1X1      y[b,co,iy,ix] = act(b'[co] + sum W'[co,ci] * x[b,ci,iy,ix]); stride 1. weight (c_out, c_in).
 *   DAL3_CONV2D_DECONV2 / _DECONV4   ConvTranspose2d(c_in, c_out, s, stride=s), s = 2 / 4 (= args.stride):
 *                        y[b,co,iy*s+dy,ix*s+dx] = act(b'[co] + sum W'[ci,co,dy,dx] * x[b,ci,iy,ix]), output (H*s, W*s).
 *                        weight (c_in, c_out, s, s).
 * act = max(., 0) with relu, the identity without. y.data is channel 0 of a tensor of y_channels channels and the layer
 * writes channels [y_channel_offset, y_channel_offset + c_out) of it: torch.cat of several layers' outputs is no copy.
 * The sums run on the fp32 MFMA (output channels on its rows, 32 output pixels on its columns, K = c_in * taps, in
 * steps of two channels per tap); the accumulator starts at b', and the ORDER of the summation is not part of the
 * definition: results are judged against a float64 evaluation (tests/rpn_ref.py). Non-finite inputs and weights are
 * outside the contract. x and y must not overlap. B, H, W <= 65535, c_in, c_out <= 4096; offsets are formed in 64 bits.
 * packed: dal3_conv2d_pack_floats(kind, c_in, c_out) floats (0 for bad arguments), 16-byte aligned; every pointer of the
 * layer is a device pointer. Invalid arguments return DAL3_EINVAL and nothing is launched. No workspace. */
enum { DAL3_CONV2D_3X3 = 0, DAL3_CONV2D_1X1 = 1, DAL3_CONV2D_DECONV2 = 2, DAL3_CONV2D_DECONV4 = 3 };

typedef struct dal3_conv2d_args {
    int32_t kind;                        /* DAL3_CONV2D_* */
    int32_t stride;                      /* 3X3: 1 or 2; 1X1: 1; DECONV2: 2; DECONV4: 4 */
    int32_t relu;                        /* 0 or 1 */
    int32_t c_in, c_out;
    int32_t y_channels;                  /* channels of the tensor y.data starts */
    int32_t y_channel_offset;            /* first channel this layer writes */
    int32_t max_workgroups;              /* 0: no cap */
    int64_t B, H, W;                     /* of the INPUT */
    dal3_map x, y;
    const float* packed;                 /* dal3_conv2d_pack's */
} dal3_conv2d_args;

size_t dal3_conv2d_pack_floats(int kind, int c_in, int c_out);
int dal3_conv2d_pack(const dal3_layer* layer, int kind, double eps, float* out, dal3_stream stream);
int dal3_conv2d(const dal3_conv2d_args* args, dal3_stream stream);

/* The same layers on 16-bit MFMA operands (v_mfma_f32_32x32x16_f16 / _bf16; additions only, nothing above changes).
 * dtype is DAL3_F16 or DAL3_BF16 at both entries; anything else returns DAL3_EINVAL and nothing is launched. The forms,
 * the strides, the channel slice, the pixel-shuffle store, max_workgroups and every limit are dal3_conv2d's. The
 * arithmetic, which is the contract:
 *   - W' of the fold above (float64, rounded once to float32) is rounded once more to the 16-bit type by
 *     dal3_conv2d_lp_pack, round to nearest even; b' stays float32;
 *   - every input activation is rounded to the 16-bit type, round to nearest even, as the kernel stages it;
 *   - the products (exact in float32: at most 22 significant bits) are summed in the MFMA's float32 accumulator, which
 *     starts at b'; ReLU and the store are float32. x and y stay float32 maps: only the OPERANDS are 16-bit.
 * As above the order of the summation is not part of the definition: a layer is judged against the float64 evaluation
 * of the ROUNDED operands under the float32 kernel's own bars, and a chain of layers against tests/rpn_lp_model.py.
 * Range: DAL3_F16 turns an activation with |x| > 65504 into an infinity, and a folded weight beyond that has no fp16
 * value: both are outside the contract, as for the DAL3_F16 point heads (the binding refuses such a weight at pack
 * time, naming the layer). DAL3_BF16 has float32's range and no such limit.
 * packed: dal3_conv2d_lp_pack_bytes(kind, c_in, c_out) bytes (0 for bad arguments), 16-byte aligned, the same for both
 * types: [float32 b' of every GEMM row, rounded up to whole tiles of 32 | 1 KiB fragments by out tile, 16 input
 * channels and tap]. A blob packed as one type must be run as that type. */
typedef struct dal3_conv2d_lp_args {
    int32_t kind;                        /* DAL3_CONV2D_* */
    int32_t stride;                      /* 3X3: 1 or 2; 1X1: 1; DECONV2: 2; DECONV4: 4 */
    int32_t relu;                        /* 0 or 1 */
    int32_t c_in, c_out;
    int32_t y_channels;                  /* channels of the tensor y.data starts */
    int32_t y_channel_offset;            /* first channel this layer writes */
    int32_t max_workgroups;              /* 0: no cap */
    int32_t dtype;                       /* DAL3_F16 | DAL3_BF16: what packed was packed as */
    int32_t reserved;                    /* 0 (anything else: DAL3_EINVAL) */
    int64_t B, H, W;                     /* of the INPUT */
    dal3_map x, y;
    const void* packed;                  /* dal3_conv2d_lp_pack's */
} dal3_conv2d_lp_args;

size_t dal3_conv2d_lp_pack_bytes(int kind, int c_in, int c_out);
int dal3_conv2d_lp_pack(const dal3_layer* layer, int kind, double eps, int dtype, void* out, dal3_stream stream);
int dal3_conv2d_lp(const dal3_conv2d_lp_args* args, dal3_stream stream);

/* ---- the backward pass of the dense stage (training the neck and the head), float32. (Additions only.) The forms, the
 * strides and the limits (B, H, W <= 65535, c_in, c_out <= 4096) are dal3_conv2d's; B, H, W, c_in and c_out are always
 * those of the layer's FORWARD input x and output y, and dy has y's extent. Every map is float32, read and written through
 * the element strides of its dal3_map with offsets formed in 64 bits: the gradient of a torch.cat is a channel-slice view
 * and a channels-last map is read as it lies; no copy of a map is made. Invalid arguments return DAL3_EINVAL and nothing
 * is launched. Built with IEEE NaN semantics. The order of every sum is a function of the argument shapes alone, there
 * are no floating-point atomics, and the bits are the same for every max_workgroups and from run to run.
 *
 * The forward in train mode needs no entry of its own: it is dal3_conv2d on the raw pack (dal3_conv2d_pack without a
 * BatchNorm, relu = 0, the convolution's own bias if it has one).
 *
 * The data gradient of DAL3_CONV2D_3X3 with stride 1 and of DAL3_CONV2D_1X1 needs no entry of its own either: it is
 * dal3_conv2d of the same form on x = dy with the pack of the transposed weight (c_in, c_out, k, k), spatially flipped
 * for 3x3 (W^T[ci,co,ky,kx] = W[co,ci,2-ky,2-kx]), without bias, BatchNorm or ReLU.
 *
 * dal3_conv2d_dgrad serves the three forms whose data gradient is no forward form:
 *   DAL3_CONV2D_3X3, stride 2     dx[b,ci,iy,ix] = sum over co, ky, kx of W[co,ci,ky,kx] * dy[b,co,(iy+1-ky)/2,(ix+1-kx)/2]
 *                                 over the taps where both divisions are exact and the output pixel exists. By the parity of
 *                                 (iy, ix) there are four phases of 1, 2, 2 and 4 taps; a workgroup's pixel grid is one
 *                                 phase's sub-grid, the phase is part of the work index (one launch), and only the taps
 *                                 that are present are multiplied.
 *   DAL3_CONV2D_DECONV2 / _DECONV4   dx[b,ci,y,x] = sum over co, dy, dx of W[ci,co,dy,dx] * g[b,co,y*s+dy,x*s+dx]: the 1x1
 *                                 form with K = c_out * s * s and a pixel-unshuffle load.
 * Any other form or stride is DAL3_EINVAL. Every element of the (B, c_in, H, W) view dx is written, +0 where nothing
 * reaches it, and nothing outside it. The sums run on the fp32 MFMA (dx channels on its rows, 32 pixels on its columns)
 * from +0; the order is not part of the definition. dy and dx must not overlap. No workspace.
 * packed: dal3_conv2d_dgrad_pack_floats(kind, c_in, c_out) floats (0 for bad arguments), 16-byte aligned, written by
 * dal3_conv2d_dgrad_pack from the parameter in its own layout ((c_out, c_in, 3, 3), or (c_in, c_out, s, s)), a device
 * pointer; there is no fold.
 *
 * dal3_conv2d_wgrad serves all five form / stride pairs and writes the gradients in the parameter's own layout:
 *   DAL3_CONV2D_3X3 / _1X1        dw[co,ci,ky,kx] = sum over b, oy, ox of dy[b,co,oy,ox] * x[b,ci,oy*s+ky-1,ox*s+kx-1], zeros
 *                                 outside the image (1x1: x[b,ci,oy,ox]);
 *   DAL3_CONV2D_DECONV2 / _DECONV4   dw[ci,co,dy,dx] = sum over b, y, x of x[b,ci,y,x] * g[b,co,y*s+dy,x*s+dx];
 *   db[co] = the sum of dy[b,co,.,.], added in float64 in a fixed order and rounded once; db may be NULL.
 * A GEMM on the fp32 MFMA with the pixels as the contraction. The pixel grid (y's for a convolution, x's for a transposed
 * one) is cut into tiles of 4 rows x TC columns (TC = 16 for DAL3_CONV2D_DECONV4, 32 otherwise), in (b, row, column)
 * order, and a slice is the DAL3_CONV2D_WGRAD_SLICE / (4 * TC) consecutive tiles that cover at most
 * DAL3_CONV2D_WGRAD_SLICE pixels. Every (32 x 32 channel tile, kernel row, slice) writes its partial sums to the
 * workspace and a second kernel adds the slices in ascending slice order. c_out of 1, 2 and 3 and every c_in up to the
 * limit are served (a tile of 32 channels is zero-padded).
 * workspace: dal3_conv2d_wgrad_workspace_bytes(kind, stride, c_in, c_out, B, H, W) bytes (0 for bad arguments), 8-byte
 * aligned: 4 * |dw| * ceil(B * ceil(PH / 4) * ceil(PW / TC) / (DAL3_CONV2D_WGRAD_SLICE / (4 * TC))), (PH, PW) the pixel
 * grid above, |dw| the parameter's element count. */
enum { DAL3_CONV2D_WGRAD_SLICE = 4096 };

typedef struct dal3_conv2d_dgrad_args {
    int32_t kind;                        /* DAL3_CONV2D_3X3 (stride 2), _DECONV2, _DECONV4 */
    int32_t stride;                      /* 3X3: 2; DECONV2: 2; DECONV4: 4 */
    int32_t c_in, c_out;                 /* of the layer */
    int32_t max_workgroups;              /* 0: no cap */
    int32_t reserved;                    /* 0 */
    int64_t B, H, W;                     /* of the layer's INPUT, which is dx's */
    dal3_map dy, dx;
    const float* packed;                 /* dal3_conv2d_dgrad_pack's */
} dal3_conv2d_dgrad_args;

typedef struct dal3_conv2d_wgrad_args {
    int32_t kind;                        /* DAL3_CONV2D_* */
    int32_t stride;                      /* 3X3: 1 or 2; 1X1: 1; DECONV2: 2; DECONV4: 4 */
    int32_t c_in, c_out;
    int32_t max_workgroups;              /* 0: no cap */
    int32_t reserved;                    /* 0 */
    int64_t B, H, W;                     /* of the layer's INPUT x */
    dal3_map x, dy;
    float* dw;                           /* the weight's own layout, contiguous */
    float* db;                           /* (c_out), or NULL */
    void* workspace;
    size_t workspace_bytes;
} dal3_conv2d_wgrad_args;

size_t dal3_conv2d_dgrad_pack_floats(int kind, int c_in, int c_out);
int dal3_conv2d_dgrad_pack(const float* weight, int kind, int c_in, int c_out, float* out, dal3_stream stream);
int dal3_conv2d_dgrad(const dal3_conv2d_dgrad_args* args, dal3_stream stream);
size_t dal3_conv2d_wgrad_workspace_bytes(int kind, int stride, int c_in, int c_out, int64_t B, int64_t H, int64_t W);
int dal3_conv2d_wgrad(const dal3_conv2d_wgrad_args* args, dal3_stream stream);

/* ---- the VoxelNet detector's sparse 3-D middle: SpMiddleResNetFHD (det3d/models/backbones/scn.py), which the reference
 * delegates to spconv 1.x: SubMConv3d (kernel 3), SparseConv3d, BatchNorm1d (folded), ReLU, SparseBasicBlock's residual and
 * the .dense().view(N, C * D, H, W) at the end. float32, eval mode. (Additions only; DAL3_VERSION stays, as for the entries
 * above.)
 *
 * A sparse tensor is features (capacity, C) float32 and indices (capacity, 4) int32 rows [b, z, y, x] on a grid
 * shape = (D, H, W) with B samples; an optional device count n (int64, 1) says that only the first min(*n, capacity) rows
 * exist. Nothing here synchronises: counts stay on the device and later kernels read them. B * D * H * W < 2^31 - 1.
 *
 * Definition. weight (kD, kH, kW, c_in, c_out), spconv 1.x's layout; a cross-correlation: output site p sums
 * in[p * stride - padding + k] @ weight[k] over the taps k whose input site is active. A submanifold layer's output sites
 * are its input sites in the same row order (kernel 3, stride 1, padding 1 in these terms). A SparseConv3d's output grid is
 * floor((in + 2 * padding - kernel) / stride) + 1 per axis; an output site is active iff an active input site lies in its
 * receptive field, and the active output sites are emitted in ascending ((b * D + z) * H + y) * W + x order.
 *
 * dal3_sp_sort: the level's (key, row) pairs sorted by key into sorted_key / sorted_pos (capacity each); rows that are no
 * site carry the key B * D * H * W at the end. A row of the first *n whose coordinates lie outside the grid or the batch
 * sets DAL3_SP_BAD_COORD and is treated as absent; equal keys set DAL3_SP_DUPLICATE (the result is then unspecified, in
 * bounds). dal3_sp_downsample: the output sites of a SparseConv3d: out_indices (out_capacity, 4) and out_key
 * (out_capacity), rows [0, *n_out) written, *n_out = min(active output sites, out_capacity); more sites than out_capacity
 * set DAL3_SP_OVERFLOW and the sites beyond it are dropped (nothing is written out of bounds and later levels stay in
 * bounds). out_capacity = min(candidates * in_capacity, B * output cells) always suffices; candidates = the product over
 * the axes of ceil(kernel / stride). dal3_sp_table: table (taps, out_capacity) int32, tap-major, tap = (kz * kH + ky) * kW
 * + kx: the row of the input site under that tap of output site i, -1 when there is none; columns [0, *n_out) are
 * written. in_key / in_pos are dal3_sp_sort's of the input (in_pos NULL: the input rows are in key order, as
 * dal3_sp_downsample emits them: its out_key). The status words are OR-ed. No atomic decides a position or a count; the
 * bytes are the same for every max_workgroups.
 *
 * dal3_sp_conv_pack folds Conv (+ optional bias) + optional eval-mode BatchNorm1d by the fold stated at the dense stage
 * ("The fold", above dal3_conv2d_pack). c_in 1 .. 8, 16, 32, 64 or 128; c_out 16, 32, 64 or 128;
 * 1 <= taps <= 27. out: dal3_sp_conv_pack_floats(taps, c_in, c_out) floats (0 for bad arguments), 16-byte aligned. A
 * folded weight that is not finite marks the pack and sets DAL3_SP_BAD_WEIGHT in *status (optional): dal3_sp_conv on
 * such a pack writes nothing and sets the same bit.
 *
 * dal3_sp_conv: y[i] = act(b' + sum over taps with table[tap][i] >= 0 of W'[tap]^T x[table[tap][i]] (+ residual[i])) for
 * i < min(*n_out, out_capacity), on the fp32 MFMA (output channels on its rows, 32 sites on its columns). An absent
 * neighbour contributes exactly zero; taps are summed in ascending order, each tap's products from zero first, so the
 * bits depend on neither the grid nor max_workgroups; there are no floating-point atomics. IEEE NaN semantics: a NaN or
 * Inf feature reaches exactly the outputs whose receptive field holds it, and act = relu keeps a NaN. center_tap >= 0
 * (a submanifold layer: 13): a row whose table entry under that tap is -1 is no site and its output row is +0. x, y and
 * residual are row-major with exactly c_in / c_out floats a row, 16-byte aligned (x: when c_in >= 16); y may be NULL with a canvas. With
 * `canvas` (canvas_B, c_out * D, H, W), canvas_shape = (D, H, W), the call first fills it with +0 on the stream and then
 * writes feature c of site (b, d, y, x) = out_indices[i] to canvas[b, c * D + d, y, x]: .dense().view(N, C * D, H, W) as a
 * store pattern. Rows whose indices fall outside the canvas are not written. Invalid arguments return DAL3_EINVAL and
 * nothing is launched. */
enum { DAL3_SP_OVERFLOW = 256, DAL3_SP_BAD_COORD = 512, DAL3_SP_DUPLICATE = 1024, DAL3_SP_BAD_WEIGHT = 2048 };  /* status bits */

typedef struct dal3_sp_sort_args {
    int64_t B;
    int32_t shape[3];                    /* D, H, W */
    int32_t reserved;                    /* 0 */
    int64_t capacity;                    /* rows of indices */
    const int64_t* n;                    /* optional device (1): rows in use */
    const int32_t* indices;              /* (capacity, 4) [b, z, y, x] */
    int32_t* sorted_key;                 /* (capacity) */
    int32_t* sorted_pos;                 /* (capacity) */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;              /* 0: no cap */
    void* workspace;
    size_t workspace_bytes;
} dal3_sp_sort_args;

typedef struct dal3_sp_downsample_args {
    int64_t B;
    int32_t in_shape[3], out_shape[3];   /* D, H, W */
    int32_t kernel[3], stride[3], padding[3];
    int32_t reserved;                    /* 0 */
    int64_t in_capacity;
    const int64_t* n_in;                 /* optional device (1) */
    const int32_t* in_indices;           /* (in_capacity, 4) */
    int64_t out_capacity;
    int32_t* out_indices;                /* (out_capacity, 4) */
    int32_t* out_key;                    /* (out_capacity) */
    int64_t* n_out;                      /* device (1) */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;
    void* workspace;
    size_t workspace_bytes;
} dal3_sp_downsample_args;

typedef struct dal3_sp_table_args {
    int64_t B;
    int32_t in_shape[3], out_shape[3];
    int32_t kernel[3], stride[3], padding[3];
    int32_t reserved;                    /* 0 */
    int64_t out_capacity;
    const int64_t* n_out;                /* optional device (1) */
    const int32_t* out_indices;          /* (out_capacity, 4) */
    int64_t in_capacity;
    const int64_t* n_in;                 /* optional device (1) */
    const int32_t* in_key;               /* (in_capacity) ascending */
    const int32_t* in_pos;               /* (in_capacity), or NULL: the identity */
    int32_t* table;                      /* (taps, out_capacity) */
    int64_t max_workgroups;
} dal3_sp_table_args;

typedef struct dal3_sp_conv_args {
    int32_t taps, c_in, c_out, relu;
    int32_t center_tap;                  /* -1, or the tap whose absence makes a row +0 */
    int32_t reserved;                    /* 0 */
    int64_t in_capacity;
    const float* x;                      /* (in_capacity, c_in) */
    int64_t out_capacity;
    const int64_t* n_out;                /* optional device (1) */
    const int32_t* table;                /* (taps, out_capacity) */
    const float* packed;                 /* dal3_sp_conv_pack's */
    const float* residual;               /* optional (out_capacity, c_out) */
    float* y;                            /* (out_capacity, c_out); may be NULL with a canvas */
    float* canvas;                       /* optional (canvas_B, c_out * D, H, W) */
    const int32_t* out_indices;          /* (out_capacity, 4), with a canvas */
    int64_t canvas_B;
    int32_t canvas_shape[3];             /* D, H, W */
    int32_t reserved2;                   /* 0 */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;
} dal3_sp_conv_args;

size_t dal3_sp_sort_workspace_bytes(int64_t capacity);
int dal3_sp_sort(const dal3_sp_sort_args* args, dal3_stream stream);
size_t dal3_sp_downsample_workspace_bytes(int64_t in_capacity, int candidates);
int dal3_sp_downsample(const dal3_sp_downsample_args* args, dal3_stream stream);
int dal3_sp_table(const dal3_sp_table_args* args, dal3_stream stream);
size_t dal3_sp_conv_pack_floats(int taps, int c_in, int c_out);
int dal3_sp_conv_pack(const dal3_layer* layer, int taps, double eps, float* out, int32_t* status, dal3_stream stream);
int dal3_sp_conv(const dal3_sp_conv_args* args, dal3_stream stream);

/* The same convolutions on 16-bit MFMA operands (v_mfma_f32_32x32x16_f16 / _bf16; additions only, nothing above changes;
 * the bookkeeping entries serve both). dtype is DAL3_F16 or DAL3_BF16 at both entries; anything else returns DAL3_EINVAL
 * and nothing is launched. The arithmetic is the dense stage's contract (above dal3_conv2d_lp_args) applied to
 * dal3_sp_conv's definition; q is one rounding to the 16-bit type, to nearest even:
 *   - W' of the fold (float64, rounded once to float32) is rounded once more, with q, by dal3_sp_conv_lp_pack; b' stays
 *     float32;
 *   - every gathered input activation is q(x). It comes one of two ways: from float32 rows `x`, rounded as they are
 *     staged, or from 16-bit rows `x16` that the producing layer stored through its `y16` = q(y), y being its float32
 *     result after residual and ReLU. Both hold the same values, so both give THE SAME OUTPUT BITS;
 *   - the products are summed in the MFMA's float32 accumulator; the order is not part of the definition, but the bits
 *     depend on neither the grid, max_workgroups nor the capacities, and there are no floating-point atomics;
 *   - the residual is float32 rows, unrounded; b', the residual, ReLU (keeps a NaN, -0 -> +0), the center_tap rule
 *     (absent -> row +0) and the canvas store are float32 and behave as in dal3_sp_conv;
 *   - an absent neighbour contributes exactly zero; a NaN or Inf feature reaches exactly the outputs whose receptive
 *     field holds it.
 * Range: DAL3_F16 turns an activation with |x| > 65504 into an infinity: outside the contract, as for the dense stage. A
 * folded weight that is not finite AFTER q marks the pack and sets DAL3_SP_BAD_WEIGHT in *status (optional); dal3_sp_conv_lp
 * on such a pack writes nothing and sets the same bit. Pack time does not synchronise.
 * Widths: dal3_sp_conv_pack's. packed: dal3_sp_conv_lp_pack_bytes(taps, c_in, c_out) bytes (0 for bad arguments), 16-byte
 * aligned, the same for both types: [64 words, the first one the flag | float32 b' of every out tile of 32 | 1 KiB
 * fragments by tap, 16 input channels and out tile]. A blob packed as one type must be run as that type.
 * The struct is dal3_sp_conv_args plus dtype, x16 and y16. Exactly one of x and x16 is non-NULL; x16 rows have c_in 16-bit
 * elements, are 16-byte aligned and need c_in 16, 32, 64 or 128 (c_in 1 .. 8 comes as float32 x only, zero-padded to one
 * k-step). y (float32 rows), y16 (c_out 16-bit elements a row, = q(y) exactly) and canvas are each optional; at least one
 * must be given. Bad combinations return DAL3_EINVAL and nothing is launched. */
typedef struct dal3_sp_conv_lp_args {
    int32_t taps, c_in, c_out, relu;
    int32_t center_tap;                  /* -1, or the tap whose absence makes a row +0 */
    int32_t reserved;                    /* 0 */
    int64_t in_capacity;
    const float* x;                      /* (in_capacity, c_in) float32, or NULL with x16 */
    int64_t out_capacity;
    const int64_t* n_out;                /* optional device (1) */
    const int32_t* table;                /* (taps, out_capacity) */
    const void* packed;                  /* dal3_sp_conv_lp_pack's */
    const float* residual;               /* optional (out_capacity, c_out) float32 */
    float* y;                            /* optional (out_capacity, c_out) */
    float* canvas;                       /* optional (canvas_B, c_out * D, H, W) */
    const int32_t* out_indices;          /* (out_capacity, 4), with a canvas */
    int64_t canvas_B;
    int32_t canvas_shape[3];             /* D, H, W */
    int32_t reserved2;                   /* 0 */
    int32_t* status;                     /* (1) OR-ed */
    int64_t max_workgroups;
    int32_t dtype;                       /* DAL3_F16 | DAL3_BF16: what packed was packed as */
    const void* x16;                     /* (in_capacity, c_in) 16-bit, or NULL with x */
    void* y16;                           /* optional (out_capacity, c_out) 16-bit */
} dal3_sp_conv_lp_args;

size_t dal3_sp_conv_lp_pack_bytes(int taps, int c_in, int c_out);
int dal3_sp_conv_lp_pack(const dal3_layer* layer, int taps, double eps, int dtype, void* out, int32_t* status, dal3_stream stream);
int dal3_sp_conv_lp(const dal3_sp_conv_lp_args* args, dal3_stream stream);

/* ---- the backward pass of the sparse convolutions (training the backbone).
 *
 * The data gradient needs no entry of its own: dx[j] = sum over taps k of dy[inv[k][j]] . W[k]^T is dal3_sp_conv with
 * x = dy, the count of the layer's INPUT, the inverse table inv (taps, in_capacity) and the pack of the transposed weight
 * (kD, kH, kW, c_out, c_in) through dal3_sp_conv_pack without bias or BatchNorm. A submanifold layer's inverse table is its
 * own table with the taps mirrored (inv[k] = table[26 - k]): pack the flipped, transposed weight and pass the forward table
 * with center_tap = 13. A SparseConv3d's comes from dal3_sp_table_transposed: table (taps, in_capacity) int32, tap-major:
 * for input site j and tap k = (kz, ky, kx) the row of the output site o = (j + padding - k) / stride, when the division is
 * exact on every axis, o lies in the output grid and is an active output site: found by lower_bound in out_key, the
 * ascending keys of dal3_sp_downsample, whose rows are in key order; -1 otherwise (a site that an overflowed level dropped
 * is simply absent). Columns [0, *n_in) are written; only the first min(*n_out, out_capacity) keys are read. No atomics;
 * the bytes are the same for every max_workgroups.
 *
 * dal3_sp_wgrad: dw[k][ci][co] = sum over i < *n_out with table[k][i] >= 0 of x[table[k][i]][ci] * dy[i][co] and
 * db[co] = sum over i < *n_out of dy[i][co], written in the parameter's own layout (kD, kH, kW, c_in, c_out) and (c_out);
 * db may be NULL. Per tap a GEMM with the sites as the contraction on the fp32 MFMA: input channels on its rows, output
 * channels on its columns, lane half h supplies site 2 s + h of k-step s, an absent neighbour supplies zeros and a k-step
 * or a tap that no site of the wave has is skipped wave-uniformly. The sites are cut into slices of
 * DAL3_SP_WGRAD_SLICE rows whatever the grid; every (tap, slice) writes its partial sums to the workspace and a second
 * kernel adds the partials of the live slices in ascending slice order: no floating-point atomics, the bits are the same
 * for every max_workgroups and from run to run. Rows of dy and table at or beyond min(*n_out, out_capacity) are never
 * read, and x is read only through the table (entries outside [0, in_capacity) count as absent). c_in 1 .. 8, 16, 32,
 * 64 or 128; c_out 16, 32, 64 or 128; 1 <= taps <= 27. x and dy are row-major with exactly c_in / c_out floats a row.
 * workspace: dal3_sp_wgrad_workspace_bytes(taps, c_in, c_out, out_capacity) bytes (0 for bad arguments), 8-byte aligned.
 * Invalid arguments return DAL3_EINVAL and nothing is launched. */
enum { DAL3_SP_WGRAD_SLICE = 1024 };

typedef struct dal3_sp_table_transposed_args {
    int64_t B;
    int32_t in_shape[3], out_shape[3];
    int32_t kernel[3], stride[3], padding[3];
    int32_t reserved;                    /* 0 */
    int64_t in_capacity;
    const int64_t* n_in;                 /* optional device (1) */
    const int32_t* in_indices;           /* (in_capacity, 4) */
    int64_t out_capacity;
    const int64_t* n_out;                /* optional device (1) */
    const int32_t* out_key;              /* (out_capacity) ascending: row r is output site r */
    int32_t* table;                      /* (taps, in_capacity) */
    int64_t max_workgroups;
} dal3_sp_table_transposed_args;

typedef struct dal3_sp_wgrad_args {
    int32_t taps, c_in, c_out;
    int32_t reserved;                    /* 0 */
    int64_t in_capacity;
    const float* x;                      /* (in_capacity, c_in): the layer's input */
    int64_t out_capacity;
    const int64_t* n_out;                /* optional device (1) */
    const int32_t* table;                /* (taps, out_capacity): the forward table */
    const float* dy;                     /* (out_capacity, c_out) */
    float* dw;                           /* (taps, c_in, c_out) */
    float* db;                           /* optional (c_out) */
    int64_t max_workgroups;
    void* workspace;
    size_t workspace_bytes;
} dal3_sp_wgrad_args;

int dal3_sp_table_transposed(const dal3_sp_table_transposed_args* args, dal3_stream stream);
size_t dal3_sp_wgrad_workspace_bytes(int taps, int c_in, int c_out, int64_t out_capacity);
int dal3_sp_wgrad(const dal3_sp_wgrad_args* args, dal3_stream stream);

/* ---- crop extraction from full sweeps: the per-detection loop of _create_pd_detection
 * (det3d/datasets/waymo/waymo_common.py:166-171, 193) for F frames at once. points (P_total,3) f32 vehicle-frame
 * sweeps concatenated, point_offsets (F+1); planes (K_total,6,4) f64 face equations of every frame's detections
 * (already in Waymo convention), box_offsets (F+1); max_points_per_frame bounds the launch. spheres (K_total,4)
 * f32 [cx,cy,cz,r^2]: a ball that CONTAINS the detection with a margin well above fp32 rounding (the library
 * culls with it before the exact test; it never decides membership; r^2 = +inf disables the cull).
 * dal3_crop_count -> counts (K_total) i64 = points inside each detection. box_start (K_total+1) = where each
 * detection's rows begin in out_points, [K_total] = the total: formed by the caller (exclusive prefix of counts) or, on
 * the device, by dal3_crop_starts -> box_start and (optional) out_offsets (K_total+1) for the detections laid out in
 * `order` (order[i] = the detection at output position i, e.g. track-major; NULL = as numbered): out_offsets[i] = rows
 * in front of position i, box_start[order[i]] = out_offsets[i]. out_points is (>= out_capacity, 3) f64; then
 * dal3_crop_fill -> out_points = veh_to_global (pose (F,16) f64 row-major) applied to the members, per detection
 * in sweep order (what `pose @ [lidars[indices]; 1]` yields); out_index (optional, i32) = index within the sweep.
 * Rows at or past out_capacity are not written (a caller that sized out_points from an estimate compares
 * box_start[K_total] with it afterwards; one that sized it from the total passes that total).
 * workspace: dal3_crop_workspace_bytes(K_total, max_points_per_frame); it carries state from count to fill. */
size_t dal3_crop_workspace_bytes(int64_t K_total, int64_t max_points_per_frame);
int dal3_crop_count(const float* points, const int64_t* point_offsets, const double* planes, const float* spheres,
                    const int64_t* box_offsets, int F, int64_t K_total, int64_t max_points_per_frame, int64_t* counts,
                    void* workspace, size_t workspace_bytes, dal3_stream stream);
int dal3_crop_fill(const float* points, const int64_t* point_offsets, const double* planes, const float* spheres,
                   const int64_t* box_offsets, int F, int64_t K_total, int64_t max_points_per_frame, const double* pose,
                   const int64_t* counts, const int64_t* box_start, double* out_points, int32_t* out_index,
                   int64_t out_capacity, const void* workspace, size_t workspace_bytes, dal3_stream stream);
int dal3_crop_starts(const int64_t* counts, const int64_t* order, int64_t K_total, int64_t* box_start,
                     int64_t* out_offsets, dal3_stream stream);
/* The same with out_offsets CAPPED at out_capacity (>= 0), for a caller that fills a buffer sized from an estimate and
 * hands (out_points, out_offsets) on to consumers that index out_points by them (dal3_static_crop_prep,
 * dal3_dynamic_item_prep): rows the fill dropped are then rows no offset points at — a detection past the capacity
 * reads as shorter or empty, never past the buffer. box_start is NOT capped: dal3_crop_fill needs the true starts, and
 * box_start[K_total] > out_capacity is how the caller learns that the buffer was too small. */
int dal3_crop_starts_capped(const int64_t* counts, const int64_t* order, int64_t K_total, int64_t* box_start,
                            int64_t* out_offsets, int64_t out_capacity, dal3_stream stream);

/* ---- training-mode building blocks of the shared-MLP stacks (first slice) --------------
 * What loss.backward() drives through Conv1d(k=1) + BatchNorm1d (batch statistics) + ReLU + max over points
 * (tools/static_model.py:271-295,326-339). Activations are POINT-MAJOR row-major fp32 (M x C), M = B*N points
 * (the memory of (B,C,N).transpose(2,1)); every channel count and M are multiples of 32 (the host pads). Each
 * layer's pre-BN output z is materialised; the consumer applies "act": y = z*scale[c] + shift[c], then max(y,0) if
 * relu_in (scale == NULL: identity). The host composes these per layer (3dal_pytorch_amd/train.py).
 *
 * dal3_tr_linear   z[p][co] (+)= sum_ci act(a[p][ci]) * Wop[co][ci] + bias.  transpose_w == 0: Wop = W, row-major
 *                  (c_out, c_in) with row stride ldw (forward); != 0: Wop[co][ci] = W[ci][co], W row-major
 *                  (c_in, c_out) (dgrad through a layer's own weight). bias: NULL | (c_out) when seg == 0 | per
 *                  segment bias[(p / seg) * c_out + co] (the decoder's per-crop global-feature term).
 * dal3_tr_colred   fixed-order column reductions over the points into out[2*C] f64:
 *                  mode 0: sum z, sum z^2 (batch statistics);
 *                  mode 1: dy = da * [act(z) > 0]: sum dy (= dbeta), sum dy * (z - mu)*rstd (= dgamma).
 *                  da: dense (M x C, row stride ldda) or NULL with (dg, arg, seg): da[p][c] = dg[s][c] if p is the
 *                  arg-max point arg[s][c] of its segment s = p / seg, else 0 (gradient of the max over points).
 * dal3_tr_bnbwd_apply  dz = k1[c] * (dy - k2[c] - xhat*k3[c])  (k1 = gamma*rstd, k2 = dbeta/M, k3 = dgamma/M).
 * dal3_tr_wgrad    dW[co][ci] = sum_p dz[p][co] * act(a[p][ci]); partial sums of point slices are added in a fixed
 *                  order (deterministic).
 * dal3_tr_segmax   g[s][c] = max_p act(z[p][c]) over segment s (relu), arg = index of the first maximum.
 * dal3_tr_segsum   out[s][c] = sum of x[p][c] over segment s. */
int dal3_tr_linear(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift, int relu_in,
                   const float* W, int64_t ldw, int transpose_w, const float* bias, int64_t seg, int c_out, float* z,
                   int64_t ldz, int accumulate, void* workspace, size_t workspace_bytes, dal3_stream stream);
size_t dal3_tr_linear_workspace_bytes(int c_in, int c_out);   /* 0 when the layer needs none (c_out % 128 != 0) */
/* dal3_tr_linear re-orders its weights into MFMA fragment order in front of every call (a ~4 us launch; a training step
 * makes 32 such calls). A caller that knows a step's layers up front packs them all — forward and transposed, the weights
 * do not change between a step's forward and backward — with ONE launch and hands each call its own image:
 *   dal3_tr_linear_pack_layout  -> the layout code (> 0) dal3_tr_linear will read for a call of this shape, 0 when that
 *                                  call uses no packed image (then pass it a plain workspace as before);
 *   dal3_tr_pack_many           packs n <= 48 layers (items: HOST array; out: device, 16-byte aligned,
 *                               dal3_tr_linear_workspace_bytes(c_in, c_out) bytes each; c_out / c_in as the CALL sees
 *                               them, i.e. swapped for transpose_w != 0);
 *   dal3_tr_linear_prepacked    dal3_tr_linear reading `packed` instead of packing. */
typedef struct {
    const float* W;
    int64_t ldw;
    int32_t transpose_w, c_out, c_in, mtb;               /* mtb: dal3_tr_linear_pack_layout() of the call */
    float* out;
} dal3_tr_pack_item;
int dal3_tr_linear_pack_layout(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, int has_act);
int dal3_tr_pack_many(const dal3_tr_pack_item* items, int n, dal3_stream stream);
int dal3_tr_linear_prepacked(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                             int relu_in, const float* W, int64_t ldw, int transpose_w, const float* bias, int64_t seg,
                             int c_out, float* z, int64_t ldz, int accumulate, const void* packed, dal3_stream stream);
/* A linear layer TOGETHER with the column reduction that follows it in a training step, taken in the kernel's epilogue
 * (round 4: the separate reduction passes re-read every activation / gradient tensor once — 1.0 of a step's 7.9 ms):
 *   dal3_tr_linear_bn_stats    = dal3_tr_linear_prepacked (forward, no accumulate) + dal3_tr_bn_stats over the first `rows`
 *                                rows of its output z;
 *   dal3_tr_linear_bnbwd_sums  = dal3_tr_linear_prepacked with transpose_w = 1, no activation, no bias (a dgrad:
 *                                da = dz W) + dal3_tr_bnbwd_sums(z = bz, da = its output): the sums of the BatchNorm/ReLU
 *                                backward of the layer whose post-activation gradient the dgrad has just produced
 *                                (bz, bscale .. brstd, gamma: that layer's pre-BN output and BatchNorm).
 * Same results as the two-call sequences up to summation order, deterministic either way. bn_stats: float64 running
 * sums per lane, a reordering of the separate pass's float64 additions (1e-6 of each vector's largest entry, the bar of
 * tests/test_gpu_train_fused.py). bnbwd_sums (RED 2): a tile's 32-64 terms of dy and dy*xhat are first added in FP32
 * (one fp32 partial per tile and channel), then joined to the float64 running sums — so dgamma / dbeta carry fp32
 * partial-sum rounding, bounded by 64 * 2^-24 = 3.8e-6 relative to sum(|terms|) per tile (the tests hold them to 1e-5 of
 * the vector's largest entry against float64 sums), not merely a reordering of float64 additions. Fused
 * when the shape takes the persistent linear kernel and rows == M (padding rows must stay out of the sums); otherwise
 * the library runs the two steps itself. Return: 1 fused, 0 ran as two steps, < 0 error.
 * workspace: dal3_tr_linear_red_workspace_bytes(rows, c_out). */
size_t dal3_tr_linear_red_workspace_bytes(int64_t rows, int c_out);
int dal3_tr_linear_bn_stats(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                            int relu_in, const float* W, int64_t ldw, const float* bias, int64_t seg, int c_out, float* z,
                            int64_t ldz, const void* packed, int64_t rows, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                            float* bn_scale, float* bn_shift, void* workspace, size_t workspace_bytes, dal3_stream stream);
int dal3_tr_linear_bnbwd_sums(const float* dz, int64_t M, int c_in, int64_t lddz, const float* W, int64_t ldw, int c_out,
                              float* da, int64_t ldda, const void* packed, int64_t rows, const float* bz, int64_t ldbz,
                              const float* bscale, const float* bshift, const float* bmu, const float* brstd,
                              const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3,
                              void* workspace, size_t workspace_bytes, dal3_stream stream);
/* The same layer on the "f16x3" arithmetic (DAL3_F16X3: fp16 MFMAs on (hi, lo) split operands, fp32 accumulate — the fp32
 * kernels' accuracy at a third of their MFMA time), for the FORWARD's big layers: operands must lie inside fp16's exponent
 * range (post-BatchNorm activations and weights do; gradients do not, so dgrad / wgrad calls stay on dal3_tr_linear).
 *   dal3_tr_linear_x3_layout -> 0 when the call does not qualify (accumulate, M % 256, c_in % 64 or > 2048, c_out % 256, seg % 256,
 *                               M < 4096), else the layout code to put into dal3_tr_pack_item.mtb for dal3_tr_pack_many
 *                               (image size: dal3_tr_linear_workspace_bytes(c_in, c_out), as for the fp32 image);
 *   dal3_tr_linear_x3           z = act(a) W^T + bias from that image. a, z, bias 16-byte aligned. */
int dal3_tr_linear_x3_layout(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, int has_act);
int dal3_tr_linear_x3(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift, int relu_in,
                      const float* bias, int64_t seg, int c_out, float* z, int64_t ldz, const void* packed,
                      const uint32_t* in_amax, dal3_stream stream);
/* ... and for an operand far below fp16's range (a dgrad's dz): in_amax (64 device words; scale must be NULL then) hold, as
 * their maximum, the bit pattern of the operand's largest |value| — what dal3_tr_bnbwd_apply_amax leaves there,
 * atomicMax'ed into 64 words the caller zeroed (64, not one: the atomics of 32,768 waves on one word take longer than
 * the layer) — and the kernel multiplies the operand by the power of two that brings that value to 2^14 and the result
 * by its inverse (both exact). Entries down to 2^-17 of the largest keep the split's 22 bits, down to 2^-28 at least 11;
 * the error stays below 1e-6 of the RESULT's range throughout. */
int dal3_tr_bnbwd_apply_amax(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda, const float* dg,
                             const int32_t* arg, int64_t seg, const float* scale, const float* shift, const float* mu,
                             const float* rstd, const float* k1, const float* k2, const float* k3, float* dz, int64_t lddz,
                             uint32_t* amax, dal3_stream stream);
/* dal3_tr_linear_pool on the same arithmetic (same arguments and workspace); _ok: 1 when the shape qualifies
 * (M % 256, c_in % 64, c_out % 256, seg % 256 == 0, M >= 4096). g / arg agree with dal3_tr_linear_pool's to the fp32 kernels'
 * accuracy (not bit for bit: the products are formed differently). */
int dal3_tr_linear_pool_x3_ok(int64_t M, int c_in, int64_t seg, int c_out);
int dal3_tr_linear_pool_x3(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift, int relu_in,
                           const float* W, int64_t ldw, const float* bias, const float* out_scale, const float* out_shift,
                           int64_t seg, int c_out, float* g, int32_t* arg, void* workspace, size_t workspace_bytes,
                           dal3_stream stream);
size_t dal3_tr_colred_workspace_bytes(int64_t M, int C);
/* out = act(x) (as dal3_tr_act_dropout without a multiplier) AND sums (2 C float64) = [sum out | sum out^2] over the M rows,
 * one pass; workspace: dal3_tr_colred_workspace_bytes(M, C). */
int dal3_tr_act_colsum(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift, int relu,
                       float* out, int64_t ldo, void* workspace, size_t workspace_bytes, double* sums, dal3_stream stream);
int dal3_tr_colred(const float* z, int64_t M, int C, int64_t ldz, int mode, const float* da, int64_t ldda,
                   const float* dg, const int32_t* arg, int64_t seg, const float* scale, const float* shift,
                   const float* mu, const float* rstd, void* workspace, size_t workspace_bytes, double* out,
                   dal3_stream stream);
/* The segmentation term of the reference's three criteria (tools/static_model.py:378-380, tools/dynamic_model.py:337-339:
 * F.nll_loss(F.log_softmax(logits.view(-1, 2), dim=1), mask_label.view(-1).long())) in one pass: loss[0] = mean over the
 * M points of -log_softmax(logits[p])[label[p]], and dlogits[p] = softmax(logits[p]) - onehot(label[p]) (the gradient
 * of M * loss; the caller scales it). logits, dlogits: (M, 2) fp32 contiguous; labels: (M,) float32 or int64 (0 / 1).
 * Sums in float64, blocks added in index order (reproducible). workspace: dal3_tr_seg_ce_workspace_bytes(M). */
size_t dal3_tr_seg_ce_workspace_bytes(int64_t M);
/* Per-channel coefficients of that backward (sums over the items in a fixed order: deterministic): with D = dg * [g > 0] and xhat = (zarg - mu) * rstd
 * (dg, g, zarg: (B, C) fp32 — upstream gradient, pooled value, pre-BN value at the pooled point), coef (4, C) float64 =
 * dbeta = sum_b D | dgamma = sum_b D xhat | A = -k1 k2 + k1 k3 rstd mu | Bc = -k1 k3 rstd  (k1 = gamma rstd, k2 = dbeta / M,
 * k3 = dgamma / M), and kd (B, C) fp32 = k1 * D. */
int dal3_tr_pool_coef(const float* dg, const float* g, const float* zarg, const float* mu, const float* rstd,
                      const float* gamma, int B, int C, int64_t M, double* coef, float* kd, dal3_stream stream);
/* The float64 algebra around that layer, K = its input channels (64, 128 or 256), C its output channels, W (C, K) row-major
 * with row stride ldw, b (C):
 *   dal3_tr_pool_moments  forward: sums (2 C) float64 = [sum z | sum z^2] of z = W a + b over M points, from m1 = sum a
 *                         (K, float64) and Sc = sum of the CENTRED a a^T (K x K fp32): mu = W m1 / M + b,
 *                         var_c = max(w_c^T (Sc / M) w_c, 0), sums = [mu M | (var + mu^2) M];
 *   dal3_tr_pool_gv       backward: G (K x K fp32) = W^T diag(Bc) W and v (K fp32) = (A + Bc b)^T W, with coef (4, C) from
 *                         dal3_tr_pool_coef — the operands of the dense part of da = a G + v;
 *   dal3_tr_pool_dw       backward: dW (C, K) fp32 = A m1^T + diag(Bc) (W S + b m1^T) + dWs, S = sum a a^T (K x K fp32)
 *                         given directly (centred = 0) or as Sc + m1 m1^T / M (centred != 0); dWs (C, K): the sparse term. */
/* zarg (B,C) = the pooled layer's pre-BatchNorm value at each pooled point: W[c] . a[b*N + arg[b][c]] + bias[c], from the
 * layer's input activation a (B*N, K) — what dal3_tr_pool_coef takes, when the fused forward (dal3_tr_linear_pool) has not
 * written the layer's output. fp32, a fixed order of additions. */
/* The FIRST layer of a stack (conv1: 3, 4 or 8 input channels -> 64 or 128) as VALU kernels, on the points as they are
 * (x: M rows of c_in floats, row stride ldx — no zero-padded copy):
 *   dal3_tr_conv1_bn_stats  z[p][c] = bias[c] + sum_k W[c][k] x[p][k] for the Mp >= M rows of z (rows >= M get x = 0), and
 *                           dal3_tr_bn_stats over the M real rows in the same pass;
 *   dal3_tr_conv1_wgrad     dW (c_out, c_in) float32, row-major: dW[c][k] = sum_{p < M} dz[p][c] x[p][k].
 * workspace: dal3_tr_conv1_workspace_bytes(rows, c_out). Float64 partial sums per 256 rows, added in a fixed order. */
size_t dal3_tr_conv1_workspace_bytes(int64_t Mp, int c_out);
int dal3_tr_conv1_bn_stats(const float* x, int64_t M, int64_t Mp, int c_in, int64_t ldx, const float* W, int64_t ldw,
                           const float* bias, int c_out, float* z, int64_t ldz, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                           float* scale, float* shift, void* workspace, size_t workspace_bytes, dal3_stream stream);
int dal3_tr_conv1_wgrad(const float* dz, int64_t lddz, const float* x, int64_t M, int c_in, int64_t ldx, int c_out, void* workspace,
                        size_t workspace_bytes, float* dW, dal3_stream stream);
/* parse_output_to_tensors (tools/static_model.py:64-92) in train mode, where its seven results must be tensors of their own:
 * the (B, 39) box_pred -> center (B,3), heading_scores (B,12), heading_residuals_normalized (B,12), heading_residuals =
 * normalized * (pi / 12), size_scores (B,3), size_residuals_normalized (B,3,3), size_residuals = normalized * MEAN_SIZE, all
 * contiguous, in one launch; _backward puts their gradients (any of them NULL = zeros) back side by side as the (B, 39)
 * gradient of box_pred: scaled gradients multiplied, then added to the normalized ones, as autograd would. */
int dal3_parse_box_pred(const float* box_pred, int64_t ldb, int64_t B, float* center, float* heading_scores,
                        float* heading_residuals_normalized, float* heading_residuals, float* size_scores,
                        float* size_residuals_normalized, float* size_residuals, dal3_stream stream);
int dal3_parse_box_pred_backward(const float* g_center, const float* g_heading_scores, const float* g_heading_residuals_normalized,
                                 const float* g_heading_residuals, const float* g_size_scores,
                                 const float* g_size_residuals_normalized, const float* g_size_residuals, int64_t B,
                                 float* g_box_pred, dal3_stream stream);
/* The per-item FC tails in train mode (static_model.py:336-338, dynamic_model.py:247-248, :284-285, :306-311;
 * `_PointHead.tail` with self.training): Linear -> BatchNorm1d over the B ITEMS -> ReLU with rows = items,
 * 2 <= B <= dal3_tr_fc_max_rows(). One launch per layer forward, two backward; no padding, no packed weight image; every
 * sum in index order (float64 for the batch statistics and the BatchNorm-backward sums).
 *   dal3_tr_fc_forward     z (B, c_out) = act(a) Wop^T + bias, act = (in_scale, in_shift, relu_in) of the layer below (NULL:
 *                          identity), Wop = W (c_out, c_in) or, transpose_w, W^T of a (c_in, c_out) matrix (the dgrad:
 *                          da_prev = dz W); with gamma != NULL also dal3_tr_bn_stats of z over its B rows (mu, rstd,
 *                          scale, shift, the running statistics when given) in the same launch
 *   dal3_tr_fc_backward_w  of the layer whose pre-BN output is z: from da (gradient w.r.t. relu(bn(z)); with scale == NULL
 *                          the layer has no BatchNorm and da IS dz) -> dz (B, c_out; may be NULL), dgamma, dbeta, db
 *                          (zeros in front of a BatchNorm), dW (c_out, c_in) = dz^T act(a_prev) (may be NULL) */
int dal3_tr_fc_max_rows(void);
int dal3_tr_fc_max_act_cin(void);       /* most input channels of a layer whose input carries an activation (hidden layers of a tail) */
int dal3_tr_fc_forward(const float* a, int64_t B, int c_in, int64_t lda, const float* in_scale, const float* in_shift, int relu_in,
                       const float* W, int64_t ldw, int transpose_w, const float* bias, int c_out, float* z, int64_t ldz,
                       const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                       float* mu, float* rstd, float* scale, float* shift, dal3_stream stream);
int dal3_tr_fc_backward_w(const float* da, int64_t ldda, int64_t B, int c_out, const float* z, int64_t ldz, const float* scale,
                          const float* shift, const float* mu, const float* rstd, const float* gamma, float* dgamma, float* dbeta,
                          const float* a_prev, int c_in, int64_t lda, const float* in_scale, const float* in_shift, int relu_in,
                          float* dz, int64_t lddz, float* dW, int64_t lddw, float* db, dal3_stream stream);
/* out (n_seg, C) = z[s*seg + arg[s][c]][c]: the same values gathered from a MATERIALISED layer output (dal3_tr_segmax's arg) */
int dal3_tr_gather_at(const float* z, int64_t ldz, const int32_t* arg, int64_t seg, int n_seg, int C, float* out,
                      dal3_stream stream);
int dal3_tr_pool_zarg(const int32_t* arg, const float* a, int64_t lda, const float* W, int64_t ldw, const float* bias, int B, int C,
                      int K, int N, float* zarg, dal3_stream stream);
int dal3_tr_pool_moments(const float* W, int64_t ldw, const float* b, const double* m1, const float* Sc, int64_t M, int C, int K,
                         double* sums, dal3_stream stream);
size_t dal3_tr_pool_gv_workspace_bytes(int K);
int dal3_tr_pool_gv(const double* coef, const float* W, int64_t ldw, const float* b, int C, int K, float* G, float* v,
                    void* workspace, size_t workspace_bytes, dal3_stream stream);
int dal3_tr_pool_dw(const double* coef, const float* W, int64_t ldw, const float* b, const float* S, const double* m1, int64_t M,
                    int centred, const float* dWs, int C, int K, float* dW, dal3_stream stream);
/* The two sparse terms of the backward of conv -> BN -> ReLU -> max over an item's N points (one pooled point per item
 * and channel: arg (B,C) int32, as dal3_tr_segmax / dal3_tr_linear_pool return it; kd (B,C) = k1 * dy at those points):
 *   da[b*N + arg[b][c]][0..K) += kd[b][c] * W[c][0..K)     in place, deterministic (channels of a point added in channel order)
 *   dWs[c][0..K) = sum over b (in order) of kd[b][c] * a[b*N + arg[b][c]][0..K)
 * K = 64, 128 or 256; 2 N + C + 1 <= 16384 and C <= 4096 (the buckets of an item live in LDS). */
int dal3_tr_pool_sparse(const int32_t* arg, const float* kd, const float* W, int64_t ldw, const float* a, int64_t lda, int B,
                        int C, int K, int N, float* da, int64_t ldda, float* dWs, dal3_stream stream);
/* The five box terms of one box estimate (tools/static_model.py:382-424, tools/dynamic_model.py:341-383), each the mean
 * over the B items: losses[0..4] = centre (Huber, delta 2, of ||center - label||), heading class (cross-entropy, 12
 * bins), heading residual (Huber, delta 1, of the label bin's normalised residual against label / (pi/12)), size class
 * (cross-entropy, 3), size residual (Huber, delta 1, of ||label / mean_size[class] - the label class's normalised
 * residual||) — unweighted; and g_* = the gradient of the matching loss w.r.t. that input (the other entries 0).
 * All inputs contiguous fp32 except the two int64 class labels. A class label outside [0, 12) / [0, 3) (an ignore value
 * such as -1: F.nll_loss of the stock criterion raises on those) makes every entry of `losses` NaN and that item's rows
 * of all five gradients NaN (a step taken on them poisons the parameters: loud whether or not the loss is looked at);
 * nothing is read out of bounds. One launch. */
int dal3_tr_box_loss(const float* center, const float* center_label, const float* heading_scores,
                     const float* heading_residuals_normalized, const int64_t* heading_class_label,
                     const float* heading_residuals_label, const float* size_scores,
                     const float* size_residuals_normalized, const int64_t* size_class_label,
                     const float* size_residuals_label, int B, float* losses, float* g_center, float* g_heading_scores,
                     float* g_heading_residuals_normalized, float* g_size_scores, float* g_size_residuals_normalized,
                     dal3_stream stream);
int dal3_tr_seg_ce(const float* logits, const void* labels, int labels_are_int64, int64_t M, float* loss, float* dlogits,
                   void* workspace, size_t workspace_bytes, dal3_stream stream);
/* The two reductions WITH their per-channel epilogues (what a training step calls: the second stage of the reduction
 * carries the epilogue, a layer's statistics are two launches): dal3_tr_bn_stats = dal3_tr_colred mode 0 followed by
 * dal3_tr_bn_finalize, dal3_tr_bnbwd_sums = mode 1 followed by dal3_tr_bnbwd_coef — same sums, same results.
 * workspace: dal3_tr_colred_workspace_bytes(M, C). */
int dal3_tr_bn_stats(const float* z, int64_t M, int C, int64_t ldz, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                     float* scale, float* shift, void* workspace, size_t workspace_bytes, dal3_stream stream);
int dal3_tr_bnbwd_sums(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda, const float* dg,
                       const int32_t* arg, int64_t seg, const float* scale, const float* shift, const float* mu,
                       const float* rstd, const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3,
                       void* workspace, size_t workspace_bytes, dal3_stream stream);
/* per-channel epilogues of the two reductions, one launch each: batch mean / biased variance -> mu, rstd, the folded
 * affine scale = gamma*rstd, shift = beta - mu*scale, and torch's running-statistics update (unbiased variance,
 * `momentum`; running_* may both be NULL); backward sums -> dgamma, dbeta and k1..k3 of dal3_tr_bnbwd_apply. */
int dal3_tr_bn_finalize(const double* sums, int C, int64_t M, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, float momentum, float eps, float* mu, float* rstd, float* scale,
                        float* shift, dal3_stream stream);
int dal3_tr_bnbwd_coef(const double* sums, int C, int64_t M, const float* gamma, const float* rstd, float* dgamma,
                       float* dbeta, float* k1, float* k2, float* k3, dal3_stream stream);
int dal3_tr_bnbwd_apply(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda, const float* dg,
                        const int32_t* arg, int64_t seg, const float* scale, const float* shift, const float* mu,
                        const float* rstd, const float* k1, const float* k2, const float* k3, float* dz, int64_t lddz,
                        dal3_stream stream);
/* dal3_tr_bnbwd_apply (dense da) that also returns the column sums of dz over every segment of sum_seg rows — seg_sums
 * (M / sum_seg, C) fp32, float64 inside, a fixed order — in the same pass: the per-crop gradient of dconv1's per-crop
 * term. C % 64 == 0, sum_seg % 128 == 0, M % sum_seg == 0. */
size_t dal3_tr_bnbwd_apply_segsum_workspace_bytes(int64_t M, int C);
int dal3_tr_bnbwd_apply_segsum(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                               const float* scale, const float* shift, const float* mu, const float* rstd, const float* k1,
                               const float* k2, const float* k3, float* dz, int64_t lddz, int64_t sum_seg, float* seg_sums,
                               void* workspace, size_t workspace_bytes, dal3_stream stream);
/* dal3_tr_wgrad on the f16x3 arithmetic (both operands split in two fp16 halves, fp32 accumulate). dz_amax: 64 device words
 * whose maximum is the bit pattern of dz's largest |value| (dal3_tr_bnbwd_apply_amax), or NULL for a dz inside fp16's
 * range. _workspace_bytes() == 0: the shape does not qualify (c_out x c_in must be cut by 256 x 256, 128 x 256, 128 x 128
 * or 512 x 64 blocks; M >= 8192) — use dal3_tr_wgrad. */
size_t dal3_tr_wgrad_x3_workspace_bytes(int64_t M, int c_out, int c_in);
int dal3_tr_wgrad_x3(const float* dz, int64_t lddz, const float* a, int64_t lda, const float* scale, const float* shift,
                     int relu_in, const uint32_t* dz_amax, int64_t M, int c_out, int c_in, void* workspace,
                     size_t workspace_bytes, float* dW, dal3_stream stream);
size_t dal3_tr_wgrad_workspace_bytes(int64_t M, int c_out, int c_in);
int dal3_tr_wgrad(const float* dz, int64_t lddz, const float* a, int64_t lda, const float* scale, const float* shift,
                  int relu_in, int64_t M, int c_out, int c_in, void* workspace, size_t workspace_bytes, float* dW,
                  dal3_stream stream);
/* dW == NULL in dal3_tr_wgrad / dal3_tr_wgrad_x3: only the per-slice partial sums are left in `workspace`
 * (dal3_tr_wgrad*_workspace_bytes / (4 c_out c_in) slices of c_out * c_in floats, which the caller keeps), and
 * dal3_tr_wgrad_final_many adds the slices of up to 24 such calls in ONE launch — the same fixed-order sums as the
 * per-call second stage (nothing reads a weight gradient before the backward pass ends). */
typedef struct dal3_tr_wgrad_part {
    const float* part;                                   /* the call's workspace */
    int64_t n_slices, n;                                 /* n = c_out * c_in */
    float* dW;
} dal3_tr_wgrad_part;
int dal3_tr_wgrad_final_many(const dal3_tr_wgrad_part* items, int n, dal3_stream stream);
int dal3_tr_segmax(const float* z, int64_t ldz, int64_t seg, int C, const float* scale, const float* shift, float* g,
                   int32_t* arg, int64_t n_seg, void* workspace /* n_seg*C*8 bytes, 8-byte aligned */,
                   size_t workspace_bytes, dal3_stream stream);
/* dal3_tr_act_dropout: out = act(x) * m, one pass. act as in dal3_tr_linear (scale == NULL: identity; relu applied after the
 * affine when relu != 0). m = mult[p][c] (row stride ldm) when mult != NULL — a caller-supplied multiplier, e.g. the
 * reference's own draw in a parity test — else m = keep / (1 - p_drop) with keep ~ Bernoulli(1 - p_drop) drawn by a
 * counter-based generator keyed on (seed, *step, element index; one draw per four consecutive elements, the keep
 * probability exact to 2^-16): forward and backward pass the same (seed, step) and get the same multiplier without storing it; step (device int64, may be NULL = 0) lets a hipGraph replay draw afresh.
 * Replaces: self.dropout = nn.Dropout(p=0.5) applied to relu(dbn4(dconv4(x))) (static_model.py:268,292-293) and its
 * backward. */
/* The 128 -> 2 logits layer with the Dropout in front of it (static_model.py:292-294: dconv5(dropout(relu(dbn4(z))))) as three
 * VALU kernels; the post-Dropout activation is never materialised, the multiplier m is re-created from its key exactly as
 * dal3_tr_act_dropout draws it (same mult / seed / step / p_drop arguments). C must be 128.
 *   dal3_tr_head2_forward  logits[p][j] = bias[j] + sum_c W[j][c] * m[p][c] * act(z[p][c])       (W: 2 rows of C, row stride ldw)
 *   dal3_tr_head2_dgrad    da[p][c] = m[p][c] * (dlogits[p][0] W[0][c] + dlogits[p][1] W[1][c])  (d / d act(z): Dropout undone)
 *   dal3_tr_head2_wgrad    dWb (258 floats): dW (2, 128) row-major, then db[0], db[1]
 *                          with dW[j][c] = sum_p dlogits[p][j] * m[p][c] * act(z[p][c]), db[j] = sum_p dlogits[p][j];
 *                          float64 partial sums per 256 rows added in a fixed order, rounded to float32 at the end.
 *                          workspace: dal3_tr_head2_wgrad_workspace_bytes(M). */
int dal3_tr_head2_forward(const float* z, int64_t M, int C, int64_t ldz, const float* scale, const float* shift, int relu,
                          const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop, const float* W,
                          int64_t ldw, const float* bias, float* logits, dal3_stream stream);
int dal3_tr_head2_dgrad(const float* dlogits, int64_t M, int C, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step,
                        float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda, dal3_stream stream);
/* dal3_tr_head2_dgrad together with dal3_tr_bnbwd_sums of the layer below (z = bz, da = the gradient just formed; the layer
 * whose relu(bn(bz)) feeds the Dropout): one kernel forms da, gates it and takes the two sums; workspace:
 * dal3_tr_colred_workspace_bytes(M, 128). Same results as the two calls up to the order of the float64 additions. */
int dal3_tr_head2_dgrad_bnbwd(const float* dlogits, int64_t M, int C, const float* mult, int64_t ldm, uint64_t seed,
                              const int64_t* step, float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda,
                              const float* bz, int64_t ldbz, const float* bscale, const float* bshift, const float* bmu,
                              const float* brstd, const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3,
                              void* workspace, size_t workspace_bytes, dal3_stream stream);
size_t dal3_tr_head2_wgrad_workspace_bytes(int64_t M);
int dal3_tr_head2_wgrad(const float* dlogits, const float* z, int64_t M, int C, int64_t ldz, const float* scale, const float* shift,
                        int relu, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop, void* workspace,
                        size_t workspace_bytes, float* dWb, dal3_stream stream);
int dal3_tr_act_dropout(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift, int relu,
                        const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop, float* out,
                        int64_t ldo, dal3_stream stream);

/* dal3_tr_linear_pool: a layer followed by BN + ReLU + max over the points of each segment, WITHOUT materialising the
 * layer's output: g[s][co] = max_p relu(z[p][co] * out_scale[co] + out_shift[co]), arg = index (within the segment) of
 * the first maximum, with z = act(a) . W^T + bias as in dal3_tr_linear (forward orientation, per-channel bias).
 * For layers whose BN affine is known before the layer runs (ins_seg's conv5, the point heads' conv4: train.py gets
 * their batch statistics from the second moments of the layer's INPUT). Bit-identical to dal3_tr_linear followed by
 * dal3_tr_segmax. c_out a multiple of 128, seg a multiple of 32 dividing M.
 * Replaces: F.relu(self.bn5(self.conv5(out4))) + torch.max(out5, 2) (static_model.py:283-284, :333-334). */
size_t dal3_tr_linear_pool_workspace_bytes(int c_in, int c_out, int64_t n_seg);
int dal3_tr_linear_pool(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift, int relu_in,
                        const float* W, int64_t ldw, const float* bias, const float* out_scale, const float* out_shift,
                        int64_t seg, int c_out, float* g, int32_t* arg, void* workspace, size_t workspace_bytes,
                        dal3_stream stream);
int dal3_tr_segsum(const float* x, int64_t ldx, int64_t seg, int C, float* out, int64_t n_seg, dal3_stream stream);

/* ---- one fused shared-MLP layer, for layer-wise tests: y = relu?(W' x + b') with BN folded,
 * x (B,C_in,N) strided -> y (B,N,C_out) point-major. */
int dal3_shared_mlp_layer(const dal3_layer* layer, int relu, dal3_bcn x, int B, int N, float* y,
                          void* workspace, size_t workspace_bytes, dal3_stream stream);
size_t dal3_shared_mlp_layer_workspace_bytes(int c_in, int c_out);

/* ---- whole-model sequencers --------------------------------------------------------------- */
typedef struct {
    int32_t B, N;                        /* crops, points per crop */
    int32_t two_stage;                   /* 0: StaticModelOneBoxEst, 1: StaticModelTwoBoxEst */
    int32_t sampler;                     /* DAL3_SAMPLER_* */
    int32_t dtype;                       /* DAL3_F32 | DAL3_BF16 | DAL3_F16: what the w_* blobs were packed as */
    int32_t reserved;
    uint64_t seed;
    int64_t item_offset;
    dal3_bcn pts;                        /* (B,3,N) logical */
    const float* init_box;               /* (B,7) */
    const float* bbox_gt;                /* (B,7) or NULL (only feeds the stage-two labels) */
    const int32_t* choice;               /* (B,512) for DAL3_SAMPLER_CHOICE, else NULL */
    const void* w_ins_seg;
    const void* w_box_est_one;           /* the only estimator when two_stage == 0 */
    const void* w_box_est_two;           /* NULL when two_stage == 0 */
    /* outputs */
    float* logits;                       /* (B,N,2) */
    uint8_t* mask;                       /* (B,N) */
    float* box_pred_one;                 /* (B,39); [:, :3] comes back with init_box[:, :3] added when two_stage */
    float* heading_residuals_one;        /* (B,12) */
    float* size_residuals_one;           /* (B,9) */
    float* center_one;                   /* (B,3) = box_pred_one[:, :3] + init_box[:, :3] */
    float* box_one;                      /* (B,7) decoded stage-one box (yaw + init yaw) */
    float* box_pred_two;                 /* two_stage only from here */
    float* heading_residuals_two;
    float* size_residuals_two;
    float* center_two;                   /* (B,3) = box_pred_two[:, :3] + center_one */
    int64_t* heading_class_label_two;    /* (B) */
    float* heading_residuals_label_two;  /* (B) */
    float* boxes7;                       /* (B,7) refined boxes (static_eval.py:269-288) */
    int32_t* counts;                     /* (B) segmented points per crop */
    int32_t* obj_idx;                    /* (B,512) */
    void* workspace;
    size_t workspace_bytes;
} dal3_static_args;

/* phases: the CHOICE sampler needs `counts` on the host between them */
enum { DAL3_PHASE_SEG = 1, DAL3_PHASE_BOX = 2, DAL3_PHASE_ALL = 3 };

size_t dal3_static_workspace_bytes(int B, int N, int two_stage);
/* StaticModelOneBoxEst.forward / StaticModelTwoBoxEst.forward (static_model.py:117-146,158-239)
 * + refined-box decode (static_eval.py:269-288) */
int dal3_static_forward(const dal3_static_args* args, int phases, dal3_stream stream);

typedef struct {
    int32_t B, N, n_box;                 /* items, points per item (5*1024), boxes per window (101) */
    int32_t sampler;
    int32_t dtype;                       /* DAL3_F32 | DAL3_BF16 | DAL3_F16 */
    int32_t reserved;
    uint64_t seed;
    int64_t item_offset;
    dal3_bcn pts;                        /* (B,4,N) logical */
    dal3_bcn box;                        /* (B,8,n_box) logical */
    const float* init_box8;              /* (B,8) or NULL: decode adds [:, :3] and yaw [:, 6] (dynamic_eval.py:236-240) */
    const int32_t* choice;               /* (B,2560) for DAL3_SAMPLER_CHOICE */
    const void* w_ins_seg;
    const void* w_point_emb;
    const void* w_box_emb;
    const void* w_box_est;
    float* logits;                       /* (B,N,2) */
    uint8_t* mask;                       /* (B,N) */
    float* embedding;                    /* (B,384) = [point_e | box_e] */
    float* box_pred;                     /* (B,39) */
    float* heading_residuals;            /* (B,12) */
    float* size_residuals;               /* (B,9) */
    float* boxes7;                       /* (B,7) */
    int32_t* counts;                     /* (B) */
    int32_t* obj_idx;                    /* (B,2560) */
    void* workspace;
    size_t workspace_bytes;
} dal3_dynamic_args;

size_t dal3_dynamic_workspace_bytes(int B, int N, int n_box);
/* DynamicModel.forward (dynamic_model.py:121-155) + decode (dynamic_eval.py:226-242) */
int dal3_dynamic_forward(const dal3_dynamic_args* args, int phases, dal3_stream stream);

/* ---- CenterPoint's second stage (det3d/models/detectors/two_stage.py, second_stage/bird_eye_view.py,
 * roi_heads/roi_head.py, roi_head_template.py): the BEV point features and the RoI head, float32, eval mode.
 * (Additions only; DAL3_VERSION stays, as for the entries above.)
 *
 * dal3_bev_gather: bilinear_interpolate_torch (det3d/core/utils/center_utils.py:92) of a BEV map at n points. The map is
 * a float32 (B, H, W, C) view by ELEMENT strides (dal3_map): the neck's NCHW tensor as it is, or an NHWC one; no copy of
 * the map is made. Point i has the absolute coordinates xy[i * xy_stride + {0, 1}] and lies in sample sample[i]
 * (sample NULL: every point in sample_index). Every operation a separately rounded float32 one, in this order:
 *   x = ((abs_x - pc_start[0]) / voxel_size[0]) / out_stride   (IEEE divisions, no reciprocal, no contraction), y likewise;
 *   x0 = floor(x), x1 = x0 + 1, both clamped to [0, W - 1]; y0, y1 likewise to [0, H - 1] (the clamp is done in float
 *   before the conversion to an index, fmax first: a NaN lands on index 0, so no coordinate reads outside the map);
 *   wa = (x1 - x) * (y1 - y), wb = (x1 - x) * (y - y0), wc = (x - x0) * (y1 - y), wd = (x - x0) * (y - y0) from the
 *   CLAMPED x0, x1, y0, y1;
 *   out[c] = ((map[y0, x0, c] * wa + map[y1, x0, c] * wb) + map[y0, x1, c] * wc) + map[y1, x1, c] * wd.
 * Everything outside the map, and on the lines x = W - 1 and y = H - 1, therefore comes out as 0 * I (two equal clamped
 * neighbours), and the result is discontinuous at coordinate 0 and at W - 1 (H - 1): the reference's behaviour, kept.
 * Point i writes C floats at out[(i / points_per_row) * out_row_stride + out_col_offset + (i % points_per_row) * C]:
 * with points_per_row 1 a call fills one section of a wider row, so the five points' sections land side by side without
 * a cat. A point whose sample lies outside [0, B) writes nothing. Outside the contract: non-finite coordinates (their
 * values; the reads stay in bounds) and relative coordinates beyond +-2^31 (the reference converts to int64 first).
 * H, W <= 65535, 1 <= C <= 65535, 1 <= points_per_row <= 5. Invalid arguments return DAL3_EINVAL and nothing is launched.
 *
 * dal3_box_points: TwoStageDetector.get_box_center for n boxes of `cols` (7 or 9) columns [x, y, z, dx, dy, ..., rot]
 * (the rotation is the LAST column): out (num_point * n, 3), section p at rows [p * n, (p + 1) * n): the centre, then
 * the front, back, left and right mid-edges ((c0 + c1) / 2, (c2 + c3) / 2, (c0 + c3) / 2, (c1 + c2) / 2) of
 * center_to_corner_box2d's corners c_k = rotation_2d((dx, dy) * ((-,-), (-,+), (+,+), (+,-)) / 2, rot) + (x, y), with
 * rotation_2d(p) = (p.x cos + p.y sin, -p.x sin + p.y cos); z is the box's. num_point 1 or 5.
 *
 * The RoI head. A dal3_roi_shape names the network: c_in = num_point * C inputs; n_shared / n_cls / n_reg (1 .. 3 each)
 * layers Conv1d(k = 1, no bias) + BatchNorm1d + ReLU of the widths shared[] / cls[] / reg[] (multiples of 16, <= 256), and
 * the two final biased Conv1d to num_class (1) and code_size (7 or 9) outputs; Dropout is the identity. dal3_roi_pack
 * takes the layers in the order shared, cls (its final layer last), reg (likewise), n_layers = n_shared + n_cls + n_reg
 * + 2, with eps[i] the BatchNorm's own (ignored for a layer without one), by the fold stated at the dense stage ("The
 * fold", above dal3_conv2d_pack); a layer's section of the blob is dal3_conv2d_pack's DAL3_CONV2D_1X1 blob of that layer.
 * out: dal3_roi_pack_floats(shape) floats (0 for a shape that is not served), 16-byte aligned.
 *
 * dal3_roi_head, the fused form (keep != NULL): from CenterHeadPost's device results (dal3_center_decode + dal3_nms: boxes
 * (K, box_cols), scores, labels, keep (F, keep_stride), keep_count (F), seg_offsets (F + 1), segment f = task * B +
 * sample, F = T * B) to the refined boxes, enqueued on the stream, nothing read back. Per sample b and slot m < M:
 *   (a) the slot's kept row: tasks in order, keep order within a task (row = seg_offsets[f] + keep[f][j]);
 *       out_counts[b] = min(kept, M); a sample with more kept rows than M sets DAL3_ROI_OVERFLOW in *status and nothing is
 *       written past M. A keep_count beyond keep_stride or a row outside [0, K) sets DAL3_NMS_BAD_SEGMENT and the slot is
 *       treated as empty. out_labels[b][m] = labels[row] + label_base[task]. Slots past the count are not computed and
 *       their outputs are not written.
 *   (b) the num_point points of dal3_box_points;  (c) dal3_bev_gather of them into the (num_point * C) feature row
 *       (out_features (B, M, num_point * C), optional: NULL keeps the rows in the workspace);
 *   (d) the MLP on the fp32 MFMA (output channels on its rows, 32 RoIs on its columns; the first layer's sum in chunks
 *       of 64 inputs, each chunk from zero; the summation order is not part of the definition, results are judged
 *       against a float64 evaluation, tests/roi_ref.py). Activations stay in LDS between the layers;
 *   (e) generate_predicted_boxes: roi = the box with the rotation moved to column 6 (code 9: columns [0..5, 8, 6, 7]);
 *       pred = reg + roi with its xyz zeroed; columns 0:3 rotated about z by roi[6] (x' = x cos + y sin, y' = -x sin +
 *       y cos, the reference's matrix); + the roi's xyz; the velocity is not rotated, the heading not wrapped;
 *   (f) post_process: out_scores = sqrt(sigmoid(cls) * score), out_boxes (B, M, code_size) with the rotation moved back
 *       to the last column (code 9: [0..5, 7, 8, 6]).
 * box_preds (B, M, code_size) / cls_preds (B, M), optional, receive (e)'s boxes before (f)'s reordering and the raw cls.
 * The direct form (keep == NULL) is RoIHead.forward: rois (B, M, code_size), roi_scores (B, M) and roi_features (B, M,
 * num_point * C) are given, every slot is computed, and steps (d) .. (f) write whichever of the outputs are not NULL.
 * dal3_roi_post is step (f) alone on n rows. box_cols must equal code_size; T <= DAL3_ROI_MAX_TASKS; B * M <= 2^24.
 * workspace: dal3_roi_head_workspace_bytes (0 for bad arguments). Anything else returns DAL3_EINVAL and launches nothing. */
enum { DAL3_ROI_OVERFLOW = 4096 };       /* status bit, numbered beside DAL3_SP_* */
#define DAL3_ROI_MAX_TASKS 16
#define DAL3_ROI_MAX_WIDTH 256

typedef struct dal3_bev_gather_args {
    int64_t B, H, W;
    int32_t C;
    int32_t sample_index;                /* every point's sample when `sample` is NULL */
    dal3_map map;
    int64_t n;                           /* points */
    const float* xy;
    int64_t xy_stride;                   /* floats between two points (>= 2) */
    const int32_t* sample;               /* (n) or NULL */
    float pc_start[2], voxel_size[2], out_stride;
    int32_t points_per_row;              /* 1 .. 5 */
    float* out;
    int64_t out_row_stride, out_col_offset;   /* in floats */
} dal3_bev_gather_args;

typedef struct dal3_roi_shape {
    int32_t c_in;                        /* num_point * C */
    int32_t n_shared, n_cls, n_reg;      /* 1 .. 3 */
    int32_t shared[3], cls[3], reg[3];
    int32_t num_class;                   /* 1 */
    int32_t code_size;                   /* 7 or 9 */
} dal3_roi_shape;

typedef struct dal3_roi_head_args {
    dal3_roi_shape shape;
    const float* packed;                 /* dal3_roi_pack's */
    int64_t B, M;
    int32_t num_point, C;
    /* the fused form */
    int32_t T, box_cols;
    int64_t K, keep_stride;
    const float* boxes;
    const float* scores;
    const int32_t* labels;
    const int32_t* keep;
    const int32_t* keep_count;
    const int64_t* seg_offsets;          /* device */
    int32_t label_base[DAL3_ROI_MAX_TASKS];
    dal3_map bev;
    int64_t H, W;
    float pc_start[2], voxel_size[2], out_stride;
    /* the direct form */
    const float* rois;
    const float* roi_scores;
    const float* roi_features;
    /* outputs, each optional */
    float* out_boxes;                    /* (B, M, code_size) */
    float* out_scores;                   /* (B, M) */
    int32_t* out_labels;                 /* (B, M); fused form */
    int32_t* out_counts;                 /* (B); fused form */
    float* out_features;                 /* (B, M, num_point * C); fused form */
    float* box_preds;                    /* (B, M, code_size) */
    float* cls_preds;                    /* (B, M) */
    int32_t* status;                     /* (1) OR-ed; fused form */
    void* workspace;
    size_t workspace_bytes;
} dal3_roi_head_args;

int dal3_bev_gather(const dal3_bev_gather_args* args, dal3_stream stream);
int dal3_box_points(const float* boxes, int64_t n, int cols, int num_point, float* out, dal3_stream stream);
size_t dal3_roi_pack_floats(const dal3_roi_shape* shape);
int dal3_roi_pack(const dal3_roi_shape* shape, const dal3_layer* layers, int n_layers, const double* eps, float* out,
                  dal3_stream stream);
size_t dal3_roi_head_workspace_bytes(int64_t B, int64_t M, int num_point, int C, int code_size);
int dal3_roi_head(const dal3_roi_head_args* args, dal3_stream stream);
int dal3_roi_post(const float* box_preds, const float* cls_preds, const float* roi_scores, int64_t n, int code_size,
                  float* out_boxes, float* out_scores, dal3_stream stream);

/* ---- The second stage's training (det3d/models/roi_heads/target_assigner/proposal_target_layer.py, roi_head_template.py):
 * target assignment and the RoI losses, float32. (Additions only; DAL3_VERSION stays.)
 *
 * dal3_roi_targets: ProposalTargetLayer.forward (SAMPLE_ROI_BY_EACH_CLASS) + RoIHeadTemplate.assign_targets for all B
 * samples in one launch, one workgroup a sample, nothing read back. Two input forms, like dal3_roi_head:
 *   fused (keep != NULL): CenterHeadPost's device results; slot m of sample b is dal3_roi_head's step (a), with the same
 *       status bits (DAL3_ROI_OVERFLOW, DAL3_NMS_BAD_SEGMENT); its label is labels[row] + label_base[task] + 1;
 *   direct: rois (B, M, code_size) with the rotation at column 6, roi_scores (B, M), roi_labels (B, M) int32.
 * A slot at or past the sample's count (direct form: a slot whose label is 0) is the reference's zero-padded RoI: zero
 * box, label 0, score 0. It takes part in the sampling as background; its sample[] is -1 and its feature row zero.
 * Per sample:
 *   GT trim: gt (B, G, code_size + 1), the box in columns 0:7, the class in the last one; trailing rows without a non-zero
 *       entry are dropped down to row 0 (rows whose non-zero entries cancel are outside the contract);
 *   overlap of RoI m: the maximum over the kept GT rows g whose class (truncated to an integer) equals the RoI's label
 *       of the 3-D intersection / max(union, 1e-6) of dal3_iou_pair.h, the LOWEST g among the maxima; (0, 0) when the
 *       class has no GT row. A NaN overlap wins, as in torch.max;
 *   subsample_rois / sample_bg_inds: fg_thresh = min(reg_fg_thresh, cls_fg_thresh); fg: overlap >= fg_thresh, easy bg:
 *       < cls_bg_thresh_lo, hard bg: < reg_fg_thresh and >= cls_bg_thresh_lo, each list ascending in m. With key =
 *       draws[b, :M] and pick = draws[b, M:] (draws (B, M + R) float32 in [0, 1)):
 *         fg and bg: the first min(fg_per_image, n_fg) of the fg list's positions p ordered by (key[p], p), then R - that
 *             many background rows; fg only: R draws from the fg list; bg only: R background rows;
 *         n background rows: hard and easy present: min((int)(n * hard_bg_ratio) [a float64 product], n_hard) hard draws,
 *             then easy draws; else n draws from the list that is not empty. Row c of the n takes pick[c];
 *         the draw from a list of n with pick v: list[min((int)(v * n), n - 1)], the product a float32 one;
 *         neither fg nor bg (NaN overlaps; the reference raises): DAL3_ROI_NO_SAMPLE in *status, the sample's rows zero,
 *             sample[] -1.
 *   Row j < R, m its sampled slot: slot[b][j] = m; sample[b][j] = b, or -1 for an empty slot; out_rois, out_labels,
 *       out_scores: the slot's; gt_iou: its overlap; gt_src: its GT row (code_size + 1); reg_valid = overlap >
 *       reg_fg_thresh; cls_labels (float): DAL3_ROI_CLS_SCORE_ROI_IOU: 1 above cls_fg_thresh, 0 below cls_bg_thresh,
 *       (overlap - cls_bg_thresh) / cls_thresh_span between; DAL3_ROI_CLS_SCORE_CLS: 1 / 0 by cls_fg_thresh, -1 strictly
 *       between the two thresholds; gt_of_rois (code_size + 1), every operation a float32 one in this order:
 *       ry = roi[6] - floor(roi[6] / 2pi + 0.5) * 2pi; e[0:6] = gt[0:6] - roi[0:6]; e[6] = gt[6] - ry; (e0, e1) rotated
 *       by -ry (x' = x cos + y sin, y' = -x sin + y cos); code 9: e[7:9] = gt[7:9] - roi[7:9], not rotated; h = e[6] mod
 *       2pi (the divisor's sign); pi/2 < h < 3pi/2: h = (h + pi) mod 2pi; h > pi: h -= 2pi; h clamped to [-pi/2, pi/2];
 *       the class column is copied. out_boxes (B, R, code_size): out_rois with the rotation back in the last column (code
 *       9: [0..5, 7, 8, 6]), the layout dal3_box_points takes: dal3_box_points on it and dal3_bev_gather with sample[]
 *       over a zeroed (B, R, num_point * C) output give the bits of dal3_roi_head's feature row of that slot.
 * M <= DAL3_ROI_TRAIN_MAX_M, 1 <= R <= DAL3_ROI_TRAIN_MAX_R, 1 <= G <= DAL3_ROI_TRAIN_MAX_G, code_size 7 or 9; non-finite boxes are outside the contract (no access leaves its array). Anything else returns DAL3_EINVAL and
 * launches nothing.
 *
 * dal3_roi_loss: get_box_cls_layer_loss (BinaryCrossEntropy) and get_box_reg_layer_loss (L1) on N rows and their gradients
 * in one launch of one workgroup, every sum in a fixed order (float64), nothing read back:
 *   cls: p = sigmoid(x); -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) summed over the rows with cls_labels >= 0,
 *       / max(count, 1), * cls_weight;
 *   reg: |reg - gt_of_rois[:, :code_size]| * code_weights over the rows with reg_valid > 0, / max(their count, 1),
 *       * reg_weight; the gradient of |.| is 0 at 0;
 *   loss[3] = (cls, reg, cls + reg); d_cls (N) and d_reg (N, code_size): the gradients of loss[2]. */
enum { DAL3_ROI_NO_SAMPLE = 8192 };      /* status bit */
enum { DAL3_ROI_CLS_SCORE_ROI_IOU = 0, DAL3_ROI_CLS_SCORE_CLS = 1 };
#define DAL3_ROI_TRAIN_MAX_M 512
#define DAL3_ROI_TRAIN_MAX_R 512
#define DAL3_ROI_TRAIN_MAX_G 1024

typedef struct dal3_roi_targets_args {
    int64_t B, M, R, G;
    int32_t code_size, reserved0;
    /* the fused form */
    int32_t T, reserved;
    int64_t K, keep_stride;
    const float* boxes;                  /* (K, code_size), the rotation last */
    const float* scores;
    const int32_t* labels;
    const int32_t* keep;
    const int32_t* keep_count;
    const int64_t* seg_offsets;          /* device */
    int32_t label_base[DAL3_ROI_MAX_TASKS];
    /* the direct form */
    const float* rois;
    const float* roi_scores;
    const int32_t* roi_labels;
    /* both */
    const float* gt;                     /* (B, G, code_size + 1) */
    const float* draws;                  /* (B, M + R) */
    int32_t fg_per_image;                /* int(round(FG_RATIO * ROI_PER_IMAGE)) */
    int32_t cls_score_type;
    float reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo;
    float cls_thresh_span;               /* (float)(CLS_FG_THRESH - CLS_BG_THRESH) */
    float reserved2;
    double hard_bg_ratio;
    /* outputs */
    int32_t* slot;                       /* (B, R) */
    int32_t* sample;                     /* (B, R) */
    float* out_rois;                     /* (B, R, code_size) */
    int32_t* out_labels;                 /* (B, R) */
    float* out_scores;                   /* (B, R) */
    float* gt_iou;                       /* (B, R) */
    float* gt_src;                       /* (B, R, code_size + 1) */
    int32_t* reg_valid;                  /* (B, R) */
    float* cls_labels;                   /* (B, R) */
    float* gt_of_rois;                   /* (B, R, code_size + 1) */
    float* out_boxes;                    /* (B, R, code_size): the rotation last */
    int32_t* status;                     /* (1) OR-ed */
} dal3_roi_targets_args;

int dal3_roi_targets(const dal3_roi_targets_args* args, dal3_stream stream);
int dal3_roi_loss(const float* rcnn_cls, const float* rcnn_reg, int64_t N, int code_size, const float* cls_labels,
                  const int32_t* reg_valid, const float* gt_of_rois, const float* code_weights /* host, code_size */,
                  float cls_weight, float reg_weight, float* loss, float* d_cls, float* d_reg, dal3_stream stream);

/* ---- The first stage's training (det3d/datasets/pipelines/preprocess.py AssignLabel, det3d/models/losses/centernet_loss.py,
 * CenterHead.loss): the head's targets and its loss with the gradients, float32. (Additions only; DAL3_VERSION stays.)
 *
 * dal3_center_targets: AssignLabel's train branch for all B samples and T tasks in one launch, nothing read back.
 *   gt (B, G, 10) is the collated gt_boxes_and_cls: x, y, z, w, l, h, rot, vx, vy, class; the class is 1-based over all
 *   tasks, a zero row is padding. Task t holds the classes (base_t, base_t + num_class[t]], base_t the sum of the counts
 *   before it. The rows of a task are taken in row order (the pipeline's flattening leaves them in the reference's per-task
 *   order); row's slot k is its rank among them. A task with more than max_objs rows sets DAL3_CENTER_OVERFLOW in *status
 *   and keeps the first max_objs (the reference asserts).
 *   A row is skipped, its slot left zero, when w <= 0 or l <= 0 in cells, or when a centre coordinate is not finite, beyond
 *   int32, or truncates (toward zero) outside [0, W) x [0, H). In float32, one operation after the other, as on the
 *   reference's float32 range and size arrays: w_c = w / voxel_size[0] / out_size_factor, l_c alike with voxel_size[1],
 *   ct = ((x, y) - pc_start) / voxel_size / out_size_factor. In float64 from those: radius = max(min_radius,
 *   (int)gaussian_radius((l_c, w_c), gaussian_overlap)), and the heat map
 *       hm[b, class, y, x] = max over the task's live objects with |x - ct_x| <= r and |y - ct_y| <= r of
 *                            (float)exp(-(dx^2 + dy^2) / (2 sigma^2)), sigma = (2 r + 1) / 6; 0 where there is none.
 *   Every pixel is written (no zero fill is needed) and is a maximum over a set: the bits do not depend on scheduling.
 *   Slot k: anno_box = ct - ct_int (2), z, log(w, l, h), vx, vy, sin(rot), cos(rot), the three functions in float64
 *   rounded once; ind = ct_y * W + ct_x; mask = 1; cat = the class within the task. Other slots are zero.
 * B <= 65535, 1 <= T <= DAL3_ROI_MAX_TASKS, 1 <= G <= 2^20, 1 <= H, W <= 65535, 1 <= max_objs <= DAL3_CENTER_MAX_OBJS,
 * 1 <= num_class <= DAL3_CENTER_MAX_CLASSES, positive voxel_size and out_size_factor, 0 <= gaussian_overlap < 1.
 * The radius must stay below 65536 cells (a box of some 10^5 cells a side; no map here is wider than 65535): a larger one,
 * or a NaN, is taken as 65536, which still covers the whole map but gives sigma, and so the values, of that radius.
 *
 * dal3_center_loss: FastFocalLoss and RegLoss of ONE task and CenterHead.loss's combination, with the gradients of `loss`
 * in every head map, from one call (three launches on the stream), nothing read back. The head maps are read in place by
 * strides. p = clamp(sigmoid(hm), 1e-4, 1 - 1e-4), its derivative zero where the clamp binds; a NaN stays a NaN.
 *   neg = sum over the map of log(1 - p) p^2 (1 - target_hm)^4; pos = sum over the slots of log(p) (1 - p)^2 mask at
 *   (ind, cat); num_pos = sum of mask over the batch; hm_loss = -(pos + neg) / num_pos, or -neg when num_pos == 0.
 *   Column c of n_cols (10 with vel, else 8: the target's velocity columns 6, 7 are dropped) over the heads reg, height,
 *   dim, [vel], rot gathered at ind: elem[c] = sum |pred mask - anno_box mask| / (num_pos + 1e-4);
 *   loc_loss = sum elem[c] code_weights[c]; loss = hm_loss + weight * loc_loss.
 *   out (4 + n_cols): loss, hm_loss, loc_loss, num_pos, elem. Elementwise terms are float32, every sum float64 in a fixed
 *   order (per-workgroup partials, then one workgroup): no floating-point atomic.
 *   grad (B, C + n_cols, H, W), every element written: d loss / d [hm | reg, height, dim, (vel), rot]. Slots that share a
 *   pixel each count once; their gradients are added in ascending slot order by one thread. sign(0) = 0.
 *   A slot whose ind or cat lies outside the map / the classes is outside the contract and is left out.
 * B, H, W as above with B * (C + n_cols) * H * W < 2^31; workspace: dal3_center_loss_workspace_bytes(B, C, H, W). */
enum { DAL3_CENTER_OVERFLOW = 16384 };   /* status bit */
#define DAL3_CENTER_MAX_OBJS 1024
#define DAL3_CENTER_MAX_CLASSES 64
#define DAL3_CENTER_MAX_COLS 10

typedef struct dal3_center_targets_args {
    int64_t B, G, H, W;
    int32_t T, max_objs;
    int32_t num_class[DAL3_ROI_MAX_TASKS];
    const float* gt;                     /* (B, G, 10) */
    float pc_start[2], voxel_size[2];
    float out_size_factor;
    int32_t min_radius;
    double gaussian_overlap;
    /* outputs, one per task */
    float* hm[DAL3_ROI_MAX_TASKS];       /* (B, num_class[t], H, W) */
    float* anno_box[DAL3_ROI_MAX_TASKS]; /* (B, max_objs, 10) */
    int64_t* ind[DAL3_ROI_MAX_TASKS];    /* (B, max_objs) */
    uint8_t* mask[DAL3_ROI_MAX_TASKS];   /* (B, max_objs) */
    int64_t* cat[DAL3_ROI_MAX_TASKS];    /* (B, max_objs) */
    int32_t* status;                     /* (1) OR-ed */
} dal3_center_targets_args;

typedef struct dal3_center_loss_args {
    int64_t B, H, W;
    int32_t C;                           /* classes of this task (hm's channels) */
    int32_t n_cols;                      /* 10 with vel, else 8 */
    int32_t max_objs, reserved;
    dal3_map hm, reg, height, dim, rot, vel;   /* logical (B, c, H, W); vel.data NULL without vel */
    const float* target_hm;              /* (B, C, H, W) */
    const float* anno_box;               /* (B, max_objs, 10) */
    const int64_t* ind;                  /* (B, max_objs) */
    const uint8_t* mask;                 /* (B, max_objs) */
    const int64_t* cat;                  /* (B, max_objs) */
    float code_weights[DAL3_CENTER_MAX_COLS];
    float weight, reserved2;
    float* out;                          /* (4 + n_cols) */
    float* grad;                         /* (B, C + n_cols, H, W) */
    void* workspace;
    size_t workspace_bytes;
} dal3_center_loss_args;

int dal3_center_targets(const dal3_center_targets_args* args, dal3_stream stream);
size_t dal3_center_loss_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int dal3_center_loss(const dal3_center_loss_args* args, dal3_stream stream);

/* ---- The training input (det3d/datasets/pipelines/preprocess.py Preprocess in train mode, Voxelization's
 * filter_gt_box_outside_range, AssignLabel's regrouping; det3d/core/sampler/sample_ops.py DataBaseSamplerV2.sample_all):
 * ground-truth paste, the global augmentation of points and boxes, the point shuffle. float32, B samples in one enqueue,
 * nothing read back. (Additions only; DAL3_VERSION stays.)
 *
 * Boxes have 9 columns x, y, z, w, l, h, vx, vy, rot. A sample has gt_counts[b] <= max_gt annotated boxes and
 * cand_counts[b] <= max_cand candidates from the object database, which the host has drawn (the integer bookkeeping of
 * sample_all) in the order of the sampler's groups: cand_group is non-decreasing within a sample. A GT class is the 1-based
 * index into class_names, 0 for a name outside it (the box still blocks a paste, and is dropped from the output), negative
 * for a name the reference removes first (DontCare, ignore, UNKNOWN: the box takes part in nothing).
 *
 * dal3_gt_paste_select: sample_class_v2 for every group of every sample, one workgroup per sample.
 *   BEV corners as center_to_corner_box2d forms them in float32 (clockwise from the minimum corner; sin and cos of the
 *   angle rounded once). Entry [i, j] of the pair matrix, candidate i against box j (the GT boxes, then the candidates), is
 *   box_collision_test's: stand-up boxes overlapping by more than 0 on both axes, then any of the sixteen edge pairs crossing
 *   by its four strict orientation tests, else every corner of one box strictly inside the other (cross >= 0 is outside).
 *   Every product and difference is one float32 rounding. The diagonal is false. coll (optional, zeroed by the caller)
 *   receives the matrix as (B, max_cand, max_gt + max_cand) bytes, the candidates' columns from max_gt on.
 *   Acceptance is the reference's serial loop: in candidate order, candidate i is rejected when it collides with a GT box,
 *   with an accepted candidate of an earlier group, or with a candidate of its own group that has not been rejected (later
 *   ones included); a rejected candidate's row and column are dead from then on. accept (B, max_cand) gets 1 / 0.
 *   The matrix is held in LDS, 40 bytes a box of the 64 KiB a workgroup declares: gt_counts[b] + cand_counts[b] <=
 *   DAL3_AUG_MAX_BOXES and cand_counts[b] <= DAL3_AUG_MAX_CAND (a column is one 64-bit word); a sample beyond that accepts
 *   nothing and sets DAL3_AUG_TOO_MANY.
 *
 * dal3_augment_points: out (n, F), n = out_offsets[B]. Sample b's source rows, indexed like its output segment
 *   [out_offsets[b], out_offsets[b + 1]), are its candidates' rows in candidate order (candidate k: rows cand_db_row[k] ..
 *   + cand_rows[k] of db_points, the first of them at source index cand_seg_start[k]; accepted or not, so the sizes are the
 *   host's) followed by its scene rows [scene_offsets[b], scene_offsets[b + 1]): the reference's order before its shuffle.
 *   Output row p is the source row of rank p - out_offsets[b] under a stable ascending sort of the sample's order keys
 *   (keys (n) int32, the low 31 bits; NULL: the identity). The ranks come from one chunked radix sort of (sample, key).
 *   A candidate's row is first moved by its box centre; the row of a rejected candidate is written as NaN in every column
 *   (dal3_voxelize drops such rows). With transform != 0 every other row then gets, each step one float32 rounding:
 *   y = -y if xform[b][0], x = -x if xform[b][1]; (x, y) = (x c + y s, -x s + y c) with s, c the float32 of sin, cos of the
 *   float64 xform[b][2]; xyz *= (float)xform[b][3]; xyz = (float)((double)xyz + xform[b][4..6]) (the reference adds a float64
 *   array to its float32 points, which NumPy evaluates in float64). Columns 3 .. F - 1 are copied. 3 <= F <= 8.
 *   A source row outside its arrays is written as NaN and sets DAL3_AUG_BAD_ROW (the device offsets disagree with the
 *   host's). workspace: dal3_augment_points_workspace_bytes(B, n); n < 2^31, B <= 65535.
 *
 * dal3_augment_boxes: gt_boxes_and_cls (B, max_objs, 10) and out_count (B), one workgroup per sample. The GT boxes, then the
 *   accepted candidates (accept NULL: none); rows whose class is outside 1 .. n_classes are dropped. With transform != 0,
 *   in the reference's order: flips (y = -y, rot = -rot + pi, vy = -vy; x = -x, rot = -rot + 2 pi, vx = -vx), rotation (xyz
 *   as the points; (vx, vy) by the float64 sine and cosine, rounded once; rot += (float)angle), columns 0 .. 7 times the
 *   scale, xyz plus the translation as for the points. Then filter_gt_box_outside_range: a box stays when one of its four
 *   BEV corners lies strictly inside minmax_to_corner_2d(range)'s polygon (range: x0, y0, x1, y1); limit_period(rot, 0.5, 2 pi);
 *   and AssignLabel's order, stable by class (its tasks partition class_names in order, so task order then class order within
 *   the task is class order, and the merged class id is the class itself). Row: x, y, z, w, l, h, rot, vx, vy, class; zero
 *   rows behind the count. More than max_objs rows keep the first max_objs and set DAL3_AUG_OVERFLOW (the reference asserts).
 *   The same limits as dal3_gt_paste_select. */
enum { DAL3_AUG_TOO_MANY = 32768, DAL3_AUG_OVERFLOW = 65536, DAL3_AUG_BAD_ROW = 131072 };   /* status bits */
#define DAL3_AUG_MAX_BOXES 1024
#define DAL3_AUG_MAX_CAND 64

typedef struct dal3_gt_paste_args {
    int64_t B;
    int32_t max_gt, max_cand;
    const float* gt_boxes;               /* (B, max_gt, 9) */
    const int32_t* gt_classes;           /* (B, max_gt) */
    const int32_t* gt_counts;            /* (B) */
    const float* cand_boxes;             /* (B, max_cand, 9) */
    const int64_t* cand_group;           /* (B, max_cand) */
    const int64_t* cand_counts;          /* (B) */
    uint8_t* accept;                     /* (B, max_cand) */
    uint8_t* coll;                       /* optional (B, max_cand, max_gt + max_cand), zeroed by the caller */
    int32_t* status;                     /* (1) OR-ed */
} dal3_gt_paste_args;

typedef struct dal3_augment_points_args {
    int64_t B, n, n_scene, db_rows;
    int32_t F, transform;
    int64_t max_cand;
    const float* scene;                  /* (n_scene, F) */
    const int64_t* scene_offsets;        /* (B + 1) */
    const float* db_points;              /* (db_rows, F) */
    const int64_t* out_offsets;          /* (B + 1) */
    const int64_t* cand_counts;          /* (B) */
    const int64_t* cand_seg_start;       /* (B, max_cand) */
    const int64_t* cand_rows;            /* (B, max_cand) */
    const int64_t* cand_db_row;          /* (B, max_cand) */
    const float* cand_boxes;             /* (B, max_cand, 9) */
    const uint8_t* accept;               /* (B, max_cand) */
    const int32_t* keys;                 /* (n) or NULL */
    const double* xform;                 /* (B, 7): flip y, flip x, rotation, scale, translation; NULL without transform */
    float* out;                          /* (n, F) */
    int32_t* status;
    int64_t max_workgroups;
    void* workspace;
    size_t workspace_bytes;
} dal3_augment_points_args;

typedef struct dal3_augment_boxes_args {
    int64_t B;
    int32_t max_gt, max_cand, max_objs, n_classes, transform, reserved;
    const float* gt_boxes;
    const int32_t* gt_classes;
    const int32_t* gt_counts;
    const float* cand_boxes;
    const int64_t* cand_classes;         /* (B, max_cand) */
    const int64_t* cand_counts;
    const uint8_t* accept;               /* NULL: no candidates */
    const double* xform;
    float range[4];
    float* out;                          /* (B, max_objs, 10) */
    int32_t* out_count;                  /* (B) */
    int32_t* status;
} dal3_augment_boxes_args;

int dal3_gt_paste_select(const dal3_gt_paste_args* args, dal3_stream stream);
size_t dal3_augment_points_workspace_bytes(int64_t B, int64_t n);
int dal3_augment_points(const dal3_augment_points_args* args, dal3_stream stream);
int dal3_augment_boxes(const dal3_augment_boxes_args* args, dal3_stream stream);

/* ---- The optimiser step (det3d/solver/fastai_optim.py OptimWrapper over torch.optim.Adam, learning_schedules_fastai.py,
 * OptimizerHook's clip_grad_norm_): Adam with decoupled or coupled weight decay, the gradient clip and a schedule table,
 * for any number of float32 parameters in two launches, nothing read back. (Additions only; DAL3_VERSION stays.)
 *
 * Storage: three flat float32 device buffers of n_flat elements, gradients, exp_avg and exp_avg_sq, with the tensors'
 * slices back to back, each slice padded to a multiple of 4 elements; the pad is zero and stays zero. The parameters stay
 * where they are: row i of the chunk table covers elements [i0, i0 + count) of one tensor, count <= DAL3_OPTIM_CHUNK, by
 * the pointer to the tensor's element i0 (i0 a multiple of DAL3_OPTIM_CHUNK) and the flat offset of the same element.
 * The hyperparameter block lives on the device; the caller writes it with ordinary stream-ordered copies.
 *
 * dal3_optim_grad_norm: partials[w] = the float64 sum of squares of the gradient elements [w S, (w + 1) S), S =
 *   DAL3_OPTIM_NORM_SPAN, in a fixed order, and hyper->step += 1 (by workgroup 0; one call per step, always before
 *   dal3_optim_step on the same stream). partials holds dal3_optim_partials(n_flat) values.
 * dal3_optim_step: with t = hyper->step, (lr, beta1) = table[min(t, total_step) - 1] when a table is attached, else the
 *   block's scalars (with a table the row taken is left in hyper->lr, hyper->beta1); every product of hyperparameters in float64, rounded to float32 once, the element arithmetic float32:
 *     DAL3_OPTIM_CLIP      c = min(1, max_norm / (sqrt(sum of partials) + 1e-6)), a NaN kept; g = g c, written back
 *                          (c == 1 keeps the bits). The sum is taken in one fixed order by every workgroup.
 *     decay rows, wd != 0  DAL3_OPTIM_TRUE_WD: p = p (1 - wd lr); otherwise g' = g + wd p (not written back)
 *     exp_avg = lerp(exp_avg, g, 1 - beta1); exp_avg_sq = exp_avg_sq beta2 + (1 - beta2) g g
 *     p = p - lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)
 *     DAL3_OPTIM_FUSED_ZERO the gradient slice is written as zeros instead
 *   IEEE semantics throughout: a non-finite gradient poisons what it poisons in torch. The norm is accumulated in float64,
 *   so gradients whose squares overflow float32 still have a finite norm here.
 * dal3_optim_total_norm: out[0] = (float)sqrt(sum of partials), the same sum as the step's. Read-only.
 * 1 <= n_chunks < 2^31, n_flat a positive multiple of 4 below 2^40, all buffers 16-byte aligned. */
#define DAL3_OPTIM_CHUNK 4096
#define DAL3_OPTIM_NORM_SPAN 16384
enum { DAL3_OPTIM_TRUE_WD = 1, DAL3_OPTIM_CLIP = 2, DAL3_OPTIM_FUSED_ZERO = 4 };   /* dal3_optim_hyper.flags */

typedef struct dal3_optim_chunk {
    float* param;                        /* the tensor's element i0 */
    int64_t offset;                      /* of the same element in the flat buffers; a multiple of 4 */
    int32_t count;                       /* 1 .. DAL3_OPTIM_CHUNK */
    int32_t decay;                       /* nonzero: weight decay applies to this tensor */
} dal3_optim_chunk;

typedef struct dal3_optim_hyper {        /* 80 bytes, every field 8 bytes wide */
    int64_t step;                        /* steps taken so far */
    double lr, beta1, beta2, eps, wd, max_norm;
    int64_t flags;                       /* DAL3_OPTIM_* */
    int64_t total_step;                  /* rows of table */
    const double* table;                 /* (total_step, 2) device: lr, beta1 of step 1, 2, ...; NULL: the scalars */
} dal3_optim_hyper;

int64_t dal3_optim_partials(int64_t n_flat);
int dal3_optim_grad_norm(const float* grad, int64_t n_flat, dal3_optim_hyper* hyper, double* partials, dal3_stream stream);
int dal3_optim_step(const dal3_optim_chunk* chunks, int64_t n_chunks, float* grad, float* exp_avg, float* exp_avg_sq,
                    int64_t n_flat, const double* partials, dal3_optim_hyper* hyper, dal3_stream stream);
int dal3_optim_total_norm(const double* partials, int64_t n_partials, float* out, dal3_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* DAL3_H */
