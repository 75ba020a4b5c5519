// dal3_api.hip — the C ABI of include/dal3.h: packed-weight layout, argument checks, sequencing of
// the kernels on the caller's stream. Host code only; no allocation, no synchronisation.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "dal3_block.h"     // Carver: the workspace carving
#include "dal3_kernels.h"
#include "dal3_lp.h"

// ---------------------------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(DAL3_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define TRY(expr)               \
    do {                        \
        int r_ = (expr);        \
        if (r_ != 0) return r_; \
    } while (0)

extern "C" int dal3_version(void) { return DAL3_VERSION; }
extern "C" const float* dal3_mean_size(void) {
    static const float v[9] = {DAL3_MEAN_SIZE_VALUES};
    return v;
}
extern "C" const char* dal3_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------- layout
static inline size_t al(size_t floats) { return (floats + 63) & ~(size_t)63; }   // 256-byte sections

struct Cursor {
    const float* base;
    size_t off;
    const float* take(size_t floats) {
        const float* p = base ? base + off : nullptr;
        off += al(floats);
        return p;
    }
    const f32x4* take4(size_t floats) { return reinterpret_cast<const f32x4*>(take(floats)); }
};

static InsSegW ins_seg_walk(Cursor& c) {
    InsSegW w;
    w.w1 = c.take(2 * 2 * 64);
    w.b1 = c.take(64);    w.b2 = c.take(64);    w.b3 = c.take(64);    w.b4 = c.take(128);   w.b5 = c.take(1024);
    w.dw1g = c.take(512 * 1024);
    w.db1 = c.take(512);  w.db2 = c.take(256);  w.db3 = c.take(128);  w.db4 = c.take(128);
    w.dw5 = c.take(2 * 128);
    w.db5 = c.take(32);
    w.enc_stream = c.take4((size_t)ENC_FRAGS * 256);
    w.dec_stream = c.take4((size_t)DEC_FRAGS * 256);
    w.lat_stream = c.take4((size_t)LAT_FRAGS * 256);
    w.w5row = c.take((size_t)1024 * 128);
    w.w5h = c.take4((size_t)32 * 4 * 2 * 256);
    w.scr_pq = c.take(2 * 1024);
    w.scr_flag = reinterpret_cast<const int32_t*>(c.take(64));
    w.dw2c = c.take((size_t)512 * 256);
    w.dw3c = c.take((size_t)256 * 128);
    w.dw4c = c.take((size_t)128 * 128);
    w.dw1c = c.take((size_t)(DEC_NULL_K + 1) * 64);
    w.w1h = c.take4((size_t)16 * 2 * 2 * 256);
    w.prn_pq = c.take(2 * 512);
    w.dec_ident = reinterpret_cast<const uint32_t*>(c.take(DEC_PLAN_LD));
    w.prn_flag = reinterpret_cast<const int32_t*>(c.take(64));
    w.dec_flag = reinterpret_cast<const int32_t*>(c.take(64));      // (stays the blob's last section)
    return w;
}

// A layout is a WALK: a function that takes the blob's sections from a Cursor, in order, and returns the struct of their
// addresses. measure() runs it on a null base (-> the sections' size in floats), view() on a packed blob.
template <class Walk, class... A>
static size_t measure(Walk walk, A... a) {
    Cursor c{nullptr, 0};
    walk(c, a...);
    return c.off;
}
template <class Walk, class... A>
static auto view(const void* base, Walk walk, A... a) {
    Cursor c{static_cast<const float*>(base), 0};
    return walk(c, a...);
}

void point_head_dims(int head_kind, int* c_in, int* ks, int c[4], int* n_fc, int fc_in[3], int fc_out[3]) {
    switch (head_kind) {
        case DAL3_HEAD_STATIC_BOX_EST:
            *c_in = 3; *ks = 2; c[0] = 128; c[1] = 128; c[2] = 256; c[3] = 512; *n_fc = 3;
            fc_in[0] = 512; fc_out[0] = 512; fc_in[1] = 512; fc_out[1] = 256; fc_in[2] = 256; fc_out[2] = 39;
            break;
        case DAL3_HEAD_POINT_EMB:
            *c_in = 4; *ks = 2; c[0] = 64; c[1] = 128; c[2] = 256; c[3] = 512; *n_fc = 2;
            fc_in[0] = 512; fc_out[0] = 512; fc_in[1] = 512; fc_out[1] = 256; fc_in[2] = 0; fc_out[2] = 0;
            break;
        default:  // DAL3_HEAD_BOX_EMB
            *c_in = 8; *ks = 4; c[0] = 64; c[1] = 64; c[2] = 128; c[3] = 512; *n_fc = 2;
            fc_in[0] = 512; fc_out[0] = 128; fc_in[1] = 128; fc_out[1] = 128; fc_in[2] = 0; fc_out[2] = 0;
            break;
    }
}

// the FC sections of a head: per layer its row-major weight, then its bias padded to 32
static FcW fc_walk(Cursor& cur, int n, const int fi[3], const int fo[3]) {
    FcW f;
    f.n = n;
    for (int i = 0; i < 3; ++i) {
        f.c_in[i] = fi[i];
        f.c_out[i] = fo[i];
        f.relu[i] = !(n == 3 && i == 2);                    // a third layer is a box estimator's output: no ReLU
        f.w[i] = i < n ? cur.take((size_t)fi[i] * fo[i]) : nullptr;
        f.b[i] = i < n ? cur.take((fo[i] + 31) / 32 * 32) : nullptr;
    }
    return f;
}

static PointHeadW point_head_walk(Cursor& cur, int head_kind) {
    int c_in, ks, c[4], n_fc, fi[3], fo[3];
    point_head_dims(head_kind, &c_in, &ks, c, &n_fc, fi, fo);
    PointHeadW w;
    w.w1 = cur.take((size_t)(c[0] / 32) * ks * 64);
    w.b1 = cur.take(c[0]);    w.b2 = cur.take(c[1]);    w.b3 = cur.take(c[2]);    w.b4 = cur.take(c[3]);
    w.stream = cur.take4(((size_t)(c[1] / 32) * (c[0] / 32) + (size_t)(c[2] / 32) * (c[1] / 32) +
                          (size_t)(c[3] / 32) * (c[2] / 32)) * 1024);
    w.fc = fc_walk(cur, n_fc, fi, fo);
    // the screened conv4's copies (heads with conv4 256 -> 512): fp32 rows, fp16 fragments, bound coefficients, flag
    const bool scr = c[2] == 256 && c[3] == 512;
    w.w4row = scr ? cur.take((size_t)512 * 256) : nullptr;
    w.w4h = scr ? cur.take4((size_t)16 * 8 * 2 * 256) : nullptr;
    w.scr_pq = scr ? cur.take(2 * 512) : nullptr;
    w.scr_flag = scr ? reinterpret_cast<const int32_t*>(cur.take(64)) : nullptr;
    return w;
}

static const int kDynFcIn[3] = {384, 128, 128}, kDynFcOut[3] = {128, 128, 39};
static FcW fc_head_walk(Cursor& cur) { return fc_walk(cur, 3, kDynFcIn, kDynFcOut); }

// ---- 16-bit and "f16x3" ins_seg (W: InsSegLpW / InsSegX3W, the same sections): fp32 sections first, then the two fragment
// streams in ring segments (f16x3: 18 / 27 segments of 32 KiB, and no dw5 in bias_dec)
template <class W>
static W ins_seg_16_walk(Cursor& c) {
    constexpr bool x3 = std::is_same<W, InsSegX3W>::value;
    W w;
    w.w1 = c.take(2 * 2 * 64);
    w.b1 = c.take(64);
    w.bias_enc = c.take(1280);
    w.bias_dec = c.take(x3 ? 608 : 864);
    w.dw1g = c.take(512 * 1024);
    w.db1 = c.take(512);
    w.enc_stream = reinterpret_cast<const uint16_t*>(c.take(x3 ? (size_t)18 * 32 * 256 : (size_t)LP_ENC_SEGS * LP_ENC_SEG * 256));
    w.dec_stream = reinterpret_cast<const uint16_t*>(c.take(x3 ? (size_t)27 * 32 * 256 : (size_t)LP_DEC_SEGS * LP_DEC_SEG * 256));
    return w;
}
static int lp_tps(int kt, int mt) { return lp_tiles_per_seg(kt, mt); }
static int point_head_lp_segments(int head_kind) {
    int c_in, ks, c[4], n_fc, fi[3], fo[3];
    point_head_dims(head_kind, &c_in, &ks, c, &n_fc, fi, fo);
    int n = 0;
    for (int l = 1; l < 4; ++l) n += (c[l] / 32) / lp_tps(c[l - 1] / 32, c[l] / 32);
    return n;
}
// ---- 16-bit and "f16x3" heads: one blob shape; the f16x3 stream holds (hi, lo) fragment pairs, padded to whole ring segments
static PointHeadLpW point_head_16_walk(Cursor& cur, int head_kind, bool x3) {
    int c_in, ks, c[4], n_fc, fi[3], fo[3];
    point_head_dims(head_kind, &c_in, &ks, c, &n_fc, fi, fo);
    PointHeadLpW w;
    w.w1 = cur.take((size_t)(c[0] / 32) * ks * 64);
    w.b1 = cur.take(c[0]);
    w.bias = cur.take(c[1] + c[2] + c[3]);
    w.fc = fc_walk(cur, n_fc, fi, fo);
    const int segs = x3 ? point_head_x3_segments(head_kind) : point_head_lp_segments(head_kind);
    w.stream = reinterpret_cast<const uint16_t*>(cur.take((size_t)segs * (x3 ? 32 : LP_HEAD_SEG) * 256));   // fragments of 256 floats
    return w;
}

// ---------------------------------------------------------------------------------- packing
static float* mut(const void* p) { return const_cast<float*>(reinterpret_cast<const float*>(p)); }

static int check_layer(const dal3_layer& L, int c_in, int c_out, const char* what) {
    if (!L.weight || !L.bias) return fail(DAL3_EINVAL, "%s: null weight/bias", what);
    if (L.c_in != c_in || L.c_out != c_out)
        return fail(DAL3_EINVAL, "%s: expected (%d -> %d), got (%d -> %d)", what, c_in, c_out, L.c_in, L.c_out);
    const bool any = L.bn_weight || L.bn_bias || L.bn_mean || L.bn_var;
    const bool all = L.bn_weight && L.bn_bias && L.bn_mean && L.bn_var;
    if (any && !all) return fail(DAL3_EINVAL, "%s: BN pointers must be all set or all NULL", what);
    return 0;
}

// fragment blocks of one layer written at fragment offset `frag` of a stream (+ its folded bias)
static int pack_frag(const dal3_layer& L, int mode, int col_off, int n_cols, const f32x4* stream, int frag,
                     const float* b, hipStream_t s, PackGroups G = PackGroups{}) {
    HIP_TRY(launch_pack_weight(L, mode, col_off, n_cols, L.c_out / 32, n_cols / 32, mut(stream) + (size_t)frag * 256, s, G));
    if (b) HIP_TRY(launch_pack_bias(L, mut(b), s));
    return 0;
}

static int pack_fc(const dal3_layer* L, const FcW& f, hipStream_t s) {
    for (int i = 0; i < f.n; ++i) {
        TRY(check_layer(L[i], f.c_in[i], f.c_out[i], "fc layer"));
        HIP_TRY(launch_pack_weight(L[i], PACK_ROWMAJOR, 0, f.c_in[i], 0, 0, mut(f.w[i]), s));
        HIP_TRY(launch_pack_bias(L[i], mut(f.b[i]), s));
    }
    return 0;
}

// what the 16-bit and the f16x3 blob of ins_seg open with (W: InsSegLpW / InsSegX3W): the fp32 first layer, the folded
// biases in the order the kernels read them, the per-crop part of dconv1. dconv5 is a row-major fp32 layer of the 16-bit
// decoder (bias_dec + 576: dw5, + 832: db5) and a fragment layer of the f16x3 one (bias_dec + 576: db5)
template <class W>
static int pack_ins_seg_16_open(const dal3_layer* L, int c_in, const W& w, bool x3, hipStream_t s) {
    float* be = mut(w.bias_enc);
    float* bd = mut(w.bias_dec);
    HIP_TRY(launch_pack_weight(L[0], PACK_FIRST, 0, c_in, 2, 2, mut(w.w1), s));
    HIP_TRY(launch_pack_bias(L[0], mut(w.b1), s));
    HIP_TRY(launch_pack_bias(L[1], be, s));
    HIP_TRY(launch_pack_bias(L[2], be + 64, s));
    HIP_TRY(launch_pack_bias(L[3], be + 128, s));
    HIP_TRY(launch_pack_bias(L[4], be + 256, s));
    HIP_TRY(launch_pack_bias(L[1], bd, s));
    HIP_TRY(launch_pack_bias(L[6], bd + 64, s));
    HIP_TRY(launch_pack_bias(L[7], bd + 320, s));
    HIP_TRY(launch_pack_bias(L[8], bd + 448, s));
    if (!x3) HIP_TRY(launch_pack_weight(L[9], PACK_ROWMAJOR, 0, 128, 0, 0, bd + 576, s));
    HIP_TRY(launch_pack_bias(L[9], bd + (x3 ? 576 : 832), s));        // db5: 2 real rows, padded to 32
    HIP_TRY(launch_pack_weight(L[5], PACK_ROWMAJOR, 64, 1024, 0, 0, mut(w.dw1g), s));
    HIP_TRY(launch_pack_bias(L[5], mut(w.db1), s));
    return 0;
}

// what every point head's blob opens with: the fp32 first layer and the folded biases of conv1 .. conv4
static int pack_head_open(const dal3_layer* L, int c_in, int ks, int c1, const float* w1, const float* b1, const float* b2,
                          const float* b3, const float* b4, hipStream_t s) {
    HIP_TRY(launch_pack_weight(L[0], PACK_FIRST, 0, c_in, c1 / 32, ks, mut(w1), s));
    HIP_TRY(launch_pack_bias(L[0], mut(b1), s));
    HIP_TRY(launch_pack_bias(L[1], mut(b2), s));
    HIP_TRY(launch_pack_bias(L[2], mut(b3), s));
    HIP_TRY(launch_pack_bias(L[3], mut(b4), s));
    return 0;
}

extern "C" int dal3_pack_weights(int head_kind, const dal3_layer* L, int n_layers, int dtype, void* packed_dev,
                                 size_t* bytes_inout, dal3_stream stream) {
    if (dtype != DAL3_F32 && dtype != DAL3_BF16 && dtype != DAL3_F16 && dtype != DAL3_F16X3)
        return fail(DAL3_EINVAL, "dal3_pack_weights: unknown dtype %d", dtype);
    if (!bytes_inout) return fail(DAL3_EINVAL, "dal3_pack_weights: bytes_inout is NULL");
    const bool x3 = dtype == DAL3_F16X3;
    const bool lp = dtype != DAL3_F32 && !x3;
    size_t floats;                                          // (the blobs a ring reads end in a tail; the 16-bit rings' do not)
    switch (head_kind) {
        case DAL3_HEAD_INS_SEG:
            floats = x3 ? measure(ins_seg_16_walk<InsSegX3W>) + DAL3_BLOB_TAIL_FLOATS
                        : lp ? measure(ins_seg_16_walk<InsSegLpW>) : measure(ins_seg_walk) + DAL3_BLOB_TAIL_FLOATS;
            break;
        case DAL3_HEAD_STATIC_BOX_EST:
        case DAL3_HEAD_POINT_EMB:
        case DAL3_HEAD_BOX_EMB:
            floats = x3 ? measure(point_head_16_walk, head_kind, true) + DAL3_BLOB_TAIL_FLOATS
                        : lp ? measure(point_head_16_walk, head_kind, false)
                             : measure(point_head_walk, head_kind) + DAL3_BLOB_TAIL_FLOATS;
            break;
        case DAL3_HEAD_DYNAMIC_BOX_EST: floats = measure(fc_head_walk); break;   // FC only: fp32 in every dtype
        default: return fail(DAL3_EINVAL, "dal3_pack_weights: unknown head_kind %d", head_kind);
    }
    const size_t need = floats * sizeof(float);
    if (!packed_dev) {
        *bytes_inout = need;
        return 0;
    }
    if (*bytes_inout < need) return fail(DAL3_EWORKSPACE, "dal3_pack_weights: need %zu bytes, got %zu", need, *bytes_inout);
    if (!L) return fail(DAL3_EINVAL, "dal3_pack_weights: layers is NULL");
    if (reinterpret_cast<uintptr_t>(packed_dev) & 255) return fail(DAL3_EINVAL, "packed_dev must be 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(packed_dev, 0, need, s));

    if (head_kind == DAL3_HEAD_INS_SEG) {
        if (n_layers != 10) return fail(DAL3_EINVAL, "ins_seg expects 10 layers, got %d", n_layers);
        const int c_in = L[0].c_in;
        if (c_in != 3 && c_in != 4) return fail(DAL3_EINVAL, "ins_seg c_in must be 3 or 4, got %d", c_in);
        static const int co[10] = {64, 64, 64, 128, 1024, 512, 256, 128, 128, 2};
        static const int ci[10] = {0, 64, 64, 64, 128, 1088, 512, 256, 128, 128};
        for (int i = 0; i < 10; ++i) TRY(check_layer(L[i], i == 0 ? c_in : ci[i], co[i], "ins_seg layer"));
        const int64_t F = 512;                                        // 16-bit elements per fragment
        if (x3) {
            const InsSegX3W w = view(packed_dev, ins_seg_16_walk<InsSegX3W>);
            uint16_t* enc = const_cast<uint16_t*>(w.enc_stream);
            uint16_t* dec = const_cast<uint16_t*>(w.dec_stream);
            TRY(pack_ins_seg_16_open(L, c_in, w, true, s));
            // encode stream (fragments): conv2 @0 (16) | conv3 @16 (16) | conv4 @32 (32) | conv5 @64 (512)
            HIP_TRY(launch_pack_weight_x3(L[1], 0, 0, 64, 2, 2, enc, s));
            HIP_TRY(launch_pack_weight_x3(L[2], 0, 0, 64, 2, 2, enc + 16 * F, s));
            HIP_TRY(launch_pack_weight_x3(L[3], 0, 0, 64, 4, 2, enc + 32 * F, s));
            HIP_TRY(launch_pack_weight_x3(L[4], 0, 0, 128, 32, 4, enc + 64 * F, s));
            // decode stream (chunks software-pipelined, dal3_pointmlp_x3.hip): conv2 @0 (16) | A_0 @16 (8) |
            // 15 x { A_{c+1} @24+40c (8), D_c @32+40c (32) } | D_15 @624 (32) | dconv3 @656 (128) | dconv4 @784 (64) |
            // dconv5 @848 (16: one out-tile, rows 0, 1 real)
            HIP_TRY(launch_pack_weight_x3(L[1], 0, 0, 64, 2, 2, dec, s));
            HIP_TRY(launch_pack_weight_x3(L[5], 0, 0, 64, 16, 2, dec, s, PackGroups{2, 16 * F, 24 * F, 40 * F}));
            HIP_TRY(launch_pack_weight_x3(L[6], 1, 0, 512, 8, 16, dec, s, PackGroups{8, 32 * F, 72 * F, 40 * F, 624 * F}));
            HIP_TRY(launch_pack_weight_x3(L[7], 0, 0, 256, 4, 8, dec + 656 * F, s));
            HIP_TRY(launch_pack_weight_x3(L[8], 0, 0, 128, 4, 4, dec + 784 * F, s));
            HIP_TRY(launch_pack_weight_x3(L[9], 0, 0, 128, 1, 4, dec + 848 * F, s));
            return 0;
        }
        if (lp) {
            const InsSegLpW w = view(packed_dev, ins_seg_16_walk<InsSegLpW>);
            uint16_t* enc = const_cast<uint16_t*>(w.enc_stream);
            uint16_t* dec = const_cast<uint16_t*>(w.dec_stream);
            TRY(pack_ins_seg_16_open(L, c_in, w, false, s));
            // encode stream (fragments): conv2 @0 | conv3 @8 | conv4 @16 | conv5 @32
            HIP_TRY(launch_pack_weight_lp(L[1], dtype, 0, 0, 64, 2, 2, enc, s));
            HIP_TRY(launch_pack_weight_lp(L[2], dtype, 0, 0, 64, 2, 2, enc + 8 * F, s));
            HIP_TRY(launch_pack_weight_lp(L[3], dtype, 0, 0, 64, 4, 2, enc + 16 * F, s));
            HIP_TRY(launch_pack_weight_lp(L[4], dtype, 0, 0, 128, 32, 4, enc + 32 * F, s));
            // decode stream, segments of 40: [conv2 @0, 1a(0) @8] ; 1a(c>=1) @40+20(c-1) ; 2(c) @44+20c ; dconv3 @360,@400 ; dconv4 @440, dconv5 @472
            HIP_TRY(launch_pack_weight_lp(L[1], dtype, 0, 0, 64, 2, 2, dec, s));
            HIP_TRY(launch_pack_weight_lp(L[5], dtype, 0, 0, 64, 16, 2, dec, s, PackGroups{2, 8 * F, 40 * F, 20 * F}));
            HIP_TRY(launch_pack_weight_lp(L[6], dtype, 1, 0, 512, 8, 16, dec, s, PackGroups{8, 44 * F, 64 * F, 20 * F}));
            HIP_TRY(launch_pack_weight_lp(L[7], dtype, 0, 0, 256, 4, 8, dec, s, PackGroups{16, 360 * F, 400 * F, 40 * F}));
            HIP_TRY(launch_pack_weight_lp(L[8], dtype, 0, 0, 128, 4, 4, dec + 440 * F, s));
            HIP_TRY(launch_pack_weight_lp(L[9], dtype, 0, 0, 128, 1, 4, dec + 472 * F, s));   // dconv5: rows 0, 1 of one out-tile
            return 0;
        }
        const InsSegW w = view(packed_dev, ins_seg_walk);
        HIP_TRY(launch_pack_weight(L[0], PACK_FIRST, 0, c_in, 2, 2, mut(w.w1), s));
        HIP_TRY(launch_pack_bias(L[0], mut(w.b1), s));
        // encode stream: conv2 | conv3 | conv4 | conv5
        TRY(pack_frag(L[1], PACK_FRAG_MT_MAJOR, 0, 64, w.enc_stream, ENC_W2, w.b2, s));
        TRY(pack_frag(L[2], PACK_FRAG_MT_MAJOR, 0, 64, w.enc_stream, ENC_W3, w.b3, s));
        TRY(pack_frag(L[3], PACK_FRAG_MT_MAJOR, 0, 64, w.enc_stream, ENC_W4, w.b4, s));
        TRY(pack_frag(L[4], PACK_FRAG_MT_MAJOR, 0, 128, w.enc_stream, ENC_W5, w.b5, s));
        // decode stream: conv2 | dconv1a(0) | { dconv1a(c+1), dconv2(c) } | dconv3 | dconv4 (fragments of 256 floats)
        TRY(pack_frag(L[1], PACK_FRAG_MT_MAJOR, 0, 64, w.dec_stream, DEC_W2, nullptr, s));
        TRY(pack_frag(L[5], PACK_FRAG_MT_MAJOR, 0, 64, w.dec_stream, DEC_MIX, w.db1, s,
                      PackGroups{/*chunk = 2 blocks*/ 2, 0, 8 * 256, 40 * 256}));          // columns of out2
        HIP_TRY(launch_pack_weight(L[5], PACK_ROWMAJOR, 64, 1024, 0, 0, mut(w.dw1g), s));   // columns of g
        TRY(pack_frag(L[6], PACK_FRAG_KT_MAJOR, 0, 512, w.dec_stream, DEC_MIX, w.db2, s,
                      PackGroups{/*chunk = 8 blocks*/ 8, 16 * 256, 56 * 256, 40 * 256}));
        TRY(pack_frag(L[7], PACK_FRAG_MT_MAJOR, 0, 256, w.dec_stream, DEC_W3, w.db3, s));
        TRY(pack_frag(L[8], PACK_FRAG_MT_MAJOR, 0, 128, w.dec_stream, DEC_W4, w.db4, s));
        // the same dconv1a / dconv2 out-tile major, for the latency kernels
        TRY(pack_frag(L[5], PACK_FRAG_MT_MAJOR, 0, 64, w.lat_stream, LAT_W1A, nullptr, s));
        TRY(pack_frag(L[6], PACK_FRAG_MT_MAJOR, 0, 512, w.lat_stream, LAT_W2, nullptr, s));
        HIP_TRY(launch_pack_weight(L[9], PACK_ROWMAJOR, 0, 128, 0, 0, mut(w.dw5), s));
        HIP_TRY(launch_pack_bias(L[9], mut(w.db5), s));
        // the screened encoder's copies of conv5: fp32 rows, fp16 fragments, per-channel error-bound coefficients
        HIP_TRY(launch_pack_weight(L[4], PACK_ROWMAJOR, 0, 128, 0, 0, mut(w.w5row), s));
        HIP_TRY(launch_pack_weight_lp(L[4], DAL3_F16, 0, 0, 128, 32, 4, reinterpret_cast<uint16_t*>(mut(w.w5h)), s));
        HIP_TRY(launch_pack_screen_bound(L[4], mut(w.scr_pq), const_cast<int32_t*>(w.scr_flag), s));
        // the compacted dconv2 - dconv4's chain-ordered copies and their guard flag
        int32_t* dec_flag = const_cast<int32_t*>(w.dec_flag);
        HIP_TRY(launch_pack_dec_chain(L[6], w.db2, mut(w.dw2c), dec_flag, s));
        HIP_TRY(launch_pack_dec_chain(L[7], w.db3, mut(w.dw3c), dec_flag, s));
        HIP_TRY(launch_pack_dec_chain(L[8], w.db4, mut(w.dw4c), dec_flag, s));
        // dconv1's crop-dead channels: the chain-ordered fp32 copy, the fp16 fragments and the bound's coefficients
        HIP_TRY(launch_pack_weight_lp(L[5], DAL3_F16, 0, 0, 64, 16, 2, reinterpret_cast<uint16_t*>(mut(w.w1h)), s));
        HIP_TRY(launch_pack_dec_prune(L[5], mut(w.dw1c), mut(w.prn_pq), const_cast<uint32_t*>(w.dec_ident),
                                      const_cast<int32_t*>(w.prn_flag), s));
        return 0;
    }
    if (head_kind == DAL3_HEAD_DYNAMIC_BOX_EST) {
        if (n_layers != 3) return fail(DAL3_EINVAL, "dynamic box_est expects 3 layers, got %d", n_layers);
        return pack_fc(L, view(packed_dev, fc_head_walk), s);
    }
    int c_in, ks, c[4], n_fc, fi[3], fo[3];
    point_head_dims(head_kind, &c_in, &ks, c, &n_fc, fi, fo);
    if (n_layers != 4 + n_fc) return fail(DAL3_EINVAL, "head %d expects %d layers, got %d", head_kind, 4 + n_fc, n_layers);
    TRY(check_layer(L[0], c_in, c[0], "conv1"));
    for (int i = 1; i < 4; ++i) TRY(check_layer(L[i], c[i - 1], c[i], "conv"));
    if (x3 || lp) {
        const PointHeadLpW w = view(packed_dev, point_head_16_walk, head_kind, x3);
        TRY(pack_head_open(L, c_in, ks, c[0], w.w1, w.b1, w.bias, w.bias + c[1], w.bias + c[1] + c[2], s));
        uint16_t* st = const_cast<uint16_t*>(w.stream);
        const int64_t SEGE = (int64_t)LP_HEAD_SEG * 512;           // 16-bit: elements per ring segment
        int64_t off = 0;
        int seg = 0;
        for (int l = 1; l < 4; ++l) {
            const int kt = c[l - 1] / 32, mt = c[l] / 32;
            if (x3) {                                              // conv2 | conv3 | conv4, out-tile major, back to back
                HIP_TRY(launch_pack_weight_x3(L[l], 0, 0, c[l - 1], mt, kt, st + off, s));
                off += (int64_t)mt * kt * 2048;
            } else {                                               // each layer: TPS out-tiles per segment
                const int tps = lp_tps(kt, mt);
                HIP_TRY(launch_pack_weight_lp(L[l], dtype, 0, 0, c[l - 1], mt, kt, st, s,
                                              PackGroups{tps * kt, seg * SEGE, (seg + 1) * SEGE, SEGE}));
                seg += mt / tps;
            }
        }
        return pack_fc(L + 4, w.fc, s);
    }
    const PointHeadW w = view(packed_dev, point_head_walk, head_kind);
    TRY(pack_head_open(L, c_in, ks, c[0], w.w1, w.b1, w.b2, w.b3, w.b4, s));
    const int f3 = (c[1] / 32) * (c[0] / 32) * 4, f4 = f3 + (c[2] / 32) * (c[1] / 32) * 4;   // fragment offsets
    TRY(pack_frag(L[1], PACK_FRAG_MT_MAJOR, 0, c[0], w.stream, 0, nullptr, s));
    TRY(pack_frag(L[2], PACK_FRAG_MT_MAJOR, 0, c[1], w.stream, f3, nullptr, s));
    TRY(pack_frag(L[3], PACK_FRAG_MT_MAJOR, 0, c[2], w.stream, f4, nullptr, s));
    if (w.w4row) {
        HIP_TRY(launch_pack_weight(L[3], PACK_ROWMAJOR, 0, 256, 0, 0, mut(w.w4row), s));
        HIP_TRY(launch_pack_weight_lp(L[3], DAL3_F16, 0, 0, 256, 16, 8, reinterpret_cast<uint16_t*>(mut(w.w4h)), s));
        HIP_TRY(launch_pack_screen_bound(L[3], mut(w.scr_pq), const_cast<int32_t*>(w.scr_flag), s));
    }
    return pack_fc(L + 4, w.fc, s);
}

static BCN to_bcn(const dal3_bcn& t) { return BCN{t.data, t.stride_b, t.stride_c, t.stride_n, t.dtype, t.flags}; }

static int check_bcn(const dal3_bcn& t, const char* what) {
    if (!t.data) return fail(DAL3_EINVAL, "%s: null data pointer", what);
    if (t.stride_n <= 0 || t.stride_c <= 0) return fail(DAL3_EINVAL, "%s: strides must be positive", what);
    if (t.dtype != DAL3_F32 && t.dtype != DAL3_BF16 && t.dtype != DAL3_F16)
        return fail(DAL3_EINVAL, "%s: storage dtype %d is none of DAL3_F32 / DAL3_BF16 / DAL3_F16", what, t.dtype);
    if (t.dtype != DAL3_F32 && (reinterpret_cast<uintptr_t>(t.data) & 1)) return fail(DAL3_EINVAL, "%s: 16-bit data must be 2-byte aligned", what);
    if (t.flags & ~(DAL3_BCN_NO_SMALL_JOB_KERNELS | DAL3_BCN_NO_WORKLIST | DAL3_BCN_NO_LDS_SAMPLER | DAL3_BCN_NO_DEC_PLAN | DAL3_BCN_NO_ENC_RESIDENT | DAL3_BCN_NO_HEAD_RESIDENT | DAL3_BCN_NO_DEC_PAIR)) return fail(DAL3_EINVAL, "%s: unknown bits in flags (%d)", what, t.flags);
    return 0;
}

// Upper bounds of a batch (dal3.h: DAL3_MAX_ITEMS, DAL3_MAX_POINTS_PER_ITEM, DAL3_MAX_TILES). The kernels index an item's
// points and the per-item outputs with 32-bit ints and launch one workgroup (or worklist entry) per 32-point tile of an
// item: a job beyond these would get a truncated grid or a wrapped offset, so it is refused here, before
// any workspace is carved or anything is launched.
static int check_extent(int64_t B, int64_t N, const char* what) {
    if (B <= 0 || N <= 0) return fail(DAL3_EINVAL, "%s: B and N must be positive (B=%lld N=%lld)", what, (long long)B, (long long)N);
    if (B > DAL3_MAX_ITEMS) return fail(DAL3_EINVAL, "%s: B=%lld items exceed DAL3_MAX_ITEMS (%d)", what, (long long)B, DAL3_MAX_ITEMS);
    if (N > DAL3_MAX_POINTS_PER_ITEM)
        return fail(DAL3_EINVAL, "%s: N=%lld points per item exceed DAL3_MAX_POINTS_PER_ITEM (%d)", what, (long long)N, DAL3_MAX_POINTS_PER_ITEM);
    if (B * ((N + 31) / 32) > (int64_t)DAL3_MAX_TILES)
        return fail(DAL3_EINVAL, "%s: B=%lld x N=%lld is %lld 32-point tiles, more than DAL3_MAX_TILES (%d): split the batch", what,
                    (long long)B, (long long)N, (long long)(B * ((N + 31) / 32)), DAL3_MAX_TILES);
    return 0;
}

// ---------------------------------------------------------------------------------- ins_seg
// prune: the encoder's maxima of dconv1a's fp16 scores; plan_*: the decoder's plan (dal3_kernels.h: DecPlan)
struct InsSegWs { float* g; float* gb; uint32_t* prune; uint32_t* plan_k; float* plan_gbc; int32_t* plan_nch; };
static InsSegWs carve_ins_seg(Carver& c, int B) {
    InsSegWs w;
    w.g = c.take<float>((size_t)B * 1024);
    w.gb = c.take<float>((size_t)B * 512);
    w.prune = c.take<uint32_t>((size_t)B * 513);
    w.plan_k = c.take<uint32_t>((size_t)B * DEC_PLAN_LD);
    w.plan_gbc = c.take<float>((size_t)B * 512);
    w.plan_nch = c.take<int32_t>((size_t)B);
    return w;
}
extern "C" size_t dal3_ins_seg_workspace_bytes(int B) {
    Carver c(nullptr, 0);
    carve_ins_seg(c, B);
    return c.off;
}

extern "C" int dal3_ins_seg_plan_layout(int B, size_t off[4], int* min_dead) {
    if (B <= 0 || !off) return fail(DAL3_EINVAL, "ins_seg_plan_layout: bad argument");
    char* const origin = reinterpret_cast<char*>(uintptr_t(4096));      // (a base that is not NULL: the carver then hands out addresses)
    Carver c(origin, ~size_t(0));
    const InsSegWs w = carve_ins_seg(c, B);
    off[0] = reinterpret_cast<char*>(w.prune) - origin, off[1] = reinterpret_cast<char*>(w.plan_k) - origin;
    off[2] = reinterpret_cast<char*>(w.plan_gbc) - origin, off[3] = reinterpret_cast<char*>(w.plan_nch) - origin;
    if (min_dead) *min_dead = DAL3_DEC_MIN_DEAD;
    return 0;
}

extern "C" int dal3_ins_seg_encoder_route(int B, int N, int flags) {
    TRY(check_extent(B, N, "ins_seg_encoder_route"));
    if (flags & ~(DAL3_BCN_NO_SMALL_JOB_KERNELS | DAL3_BCN_NO_WORKLIST | DAL3_BCN_NO_LDS_SAMPLER | DAL3_BCN_NO_DEC_PLAN | DAL3_BCN_NO_ENC_RESIDENT | DAL3_BCN_NO_HEAD_RESIDENT | DAL3_BCN_NO_DEC_PAIR))
        return fail(DAL3_EINVAL, "ins_seg_encoder_route: unknown bits in flags (%d)", flags);
    return enc_route(flags, B, N);
}

extern "C" int dal3_ins_seg_decode_route(const void* packed, int B, int N, int flags) {
    TRY(check_extent(B, N, "ins_seg_decode_route"));
    if (flags & ~(DAL3_BCN_NO_SMALL_JOB_KERNELS | DAL3_BCN_NO_WORKLIST | DAL3_BCN_NO_LDS_SAMPLER | DAL3_BCN_NO_DEC_PLAN | DAL3_BCN_NO_ENC_RESIDENT | DAL3_BCN_NO_HEAD_RESIDENT | DAL3_BCN_NO_DEC_PAIR))
        return fail(DAL3_EINVAL, "ins_seg_decode_route: unknown bits in flags (%d)", flags);
    int32_t guard = 0;
    if (packed) HIP_TRY(hipMemcpy(&guard, view(packed, ins_seg_walk).dec_flag, sizeof(guard), hipMemcpyDeviceToHost));
    return dec_route(flags, B, N, guard != 0);
}

static int check_dtype(int dtype) {
    if (dtype != DAL3_F32 && dtype != DAL3_BF16 && dtype != DAL3_F16 && dtype != DAL3_F16X3)
        return fail(DAL3_EINVAL, "unknown dtype %d", dtype);
    return 0;
}

static int ins_seg_run(const void* packed, int dtype, int c_in, const dal3_bcn& pts, int B, int N, float* logits,
                       uint8_t* mask, float* global_feat_out, const InsSegWs& ws, hipStream_t s) {
    TRY(check_dtype(dtype));
    if (!packed || !logits || !mask) return fail(DAL3_EINVAL, "ins_seg: null pointer");
    TRY(check_extent(B, N, "ins_seg"));
    if (c_in != 3 && c_in != 4) return fail(DAL3_EINVAL, "ins_seg: c_in must be 3 or 4");
    TRY(check_bcn(pts, "pts"));
    const BCN x = to_bcn(pts);
    HIP_TRY(launch_nonfinite_rows(x, B, N, c_in, ws.g, 1024, s));      // g = 0 (NaN for a crop with a non-finite coordinate)
    if (dtype == DAL3_F32) {
        const InsSegW w = view(packed, ins_seg_walk);
        // the screened encoder and the compacted decoder both run: dconv1's channels that are dead for a whole crop are
        // proved so from the encoder's fp16 maxima and the decoder leaves them out (DESIGN.md "Crop-dead channels of dconv1")
        const bool plan = dec_plan_route(x.flags, B, N);
        if (plan) HIP_TRY(hipMemsetAsync(ws.prune, 0, (size_t)B * 513 * sizeof(uint32_t), s));
        HIP_TRY(launch_ins_seg_encode(w, x, c_in, B, N, ws.g, s, plan ? ws.prune : nullptr));
        // per-crop part of dconv1: gb = W1g' . g + b1'   (static_model.py:286-289 without the repeat+cat)
        HIP_TRY(launch_fc(w.dw1g, w.db1, ws.g, 1024, ws.gb, 512, B, 1024, 512, 0, s));
        if (plan) HIP_TRY(launch_dec_plan(w, ws.gb, ws.prune, B, ws.plan_k, ws.plan_gbc, ws.plan_nch, s));
        HIP_TRY(launch_ins_seg_decode(w, x, c_in, B, N, ws.gb, logits, mask, s,
                                      plan ? DecPlan{ws.plan_k, ws.plan_gbc, ws.plan_nch} : DecPlan{nullptr, nullptr, nullptr}));
    } else if (dtype == DAL3_F16X3) {
        const InsSegX3W w = view(packed, ins_seg_16_walk<InsSegX3W>);
        HIP_TRY(launch_ins_seg_encode_x3(w, x, c_in, B, N, ws.g, s));
        HIP_TRY(launch_fc(w.dw1g, w.db1, ws.g, 1024, ws.gb, 512, B, 1024, 512, 0, s));
        HIP_TRY(launch_ins_seg_decode_x3(w, x, c_in, B, N, ws.gb, logits, mask, s));
    } else {
        const InsSegLpW w = view(packed, ins_seg_16_walk<InsSegLpW>);
        HIP_TRY(launch_ins_seg_encode_lp(dtype, w, x, c_in, B, N, ws.g, s));
        HIP_TRY(launch_fc(w.dw1g, w.db1, ws.g, 1024, ws.gb, 512, B, 1024, 512, 0, s));
        HIP_TRY(launch_ins_seg_decode_lp(dtype, w, x, c_in, B, N, ws.gb, logits, mask, s));
    }
    if (global_feat_out)
        HIP_TRY(hipMemcpyAsync(global_feat_out, ws.g, (size_t)B * 1024 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

extern "C" int dal3_ins_seg_forward(const void* packed, int dtype, int c_in, dal3_bcn pts, int B, int N, float* logits,
                                    uint8_t* mask, float* global_feat_out, void* workspace, size_t workspace_bytes,
                                    dal3_stream stream) {
    if (!workspace) return fail(DAL3_EINVAL, "ins_seg: workspace is NULL");
    TRY(check_extent(B, N, "ins_seg"));
    Carver c(workspace, workspace_bytes);
    const InsSegWs ws = carve_ins_seg(c, B);
    if (!c.ok) return fail(DAL3_EWORKSPACE, "ins_seg: workspace needs %zu bytes, got %zu", c.off, workspace_bytes);
    return ins_seg_run(packed, dtype, c_in, pts, B, N, logits, mask, global_feat_out, ws, static_cast<hipStream_t>(stream));
}

extern "C" int dal3_ins_seg_encode(const void* packed, int dtype, int c_in, dal3_bcn pts, int B, int N,
                                   float* global_feat, dal3_stream stream) {
    TRY(check_dtype(dtype));
    if (!packed || !global_feat || (c_in != 3 && c_in != 4)) return fail(DAL3_EINVAL, "ins_seg_encode: bad argument");
    TRY(check_extent(B, N, "ins_seg_encode"));
    TRY(check_bcn(pts, "pts"));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == DAL3_F32)
        HIP_TRY(launch_ins_seg_encode(view(packed, ins_seg_walk), to_bcn(pts), c_in, B, N,
                                      global_feat, s));
    else if (dtype == DAL3_F16X3)
        HIP_TRY(launch_ins_seg_encode_x3(view(packed, ins_seg_16_walk<InsSegX3W>), to_bcn(pts), c_in, B, N, global_feat, s));
    else
        HIP_TRY(launch_ins_seg_encode_lp(dtype, view(packed, ins_seg_16_walk<InsSegLpW>), to_bcn(pts), c_in, B, N, global_feat, s));
    return 0;
}

extern "C" int dal3_ins_seg_global_bias(const void* packed, int dtype, const float* global_feat, int B, float* gbias,
                                        dal3_stream stream) {
    TRY(check_dtype(dtype));
    if (!packed || !global_feat || !gbias) return fail(DAL3_EINVAL, "ins_seg_global_bias: bad argument");
    TRY(check_extent(B, 1, "ins_seg_global_bias"));
    const float *dw1g, *db1;                                // (the same two sections of every dtype's blob)
    auto sections = [&](const auto& w) { dw1g = w.dw1g, db1 = w.db1; };
    if (dtype == DAL3_F32) sections(view(packed, ins_seg_walk));
    else if (dtype == DAL3_F16X3) sections(view(packed, ins_seg_16_walk<InsSegX3W>));
    else sections(view(packed, ins_seg_16_walk<InsSegLpW>));
    HIP_TRY(launch_fc(dw1g, db1, global_feat, 1024, gbias, 512, B, 1024, 512, 0, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_ins_seg_decode(const void* packed, int dtype, int c_in, dal3_bcn pts, int B, int N,
                                   const float* gbias, float* logits, uint8_t* mask, dal3_stream stream) {
    TRY(check_dtype(dtype));
    if (!packed || !gbias || !logits || !mask || (c_in != 3 && c_in != 4)) return fail(DAL3_EINVAL, "ins_seg_decode: bad argument");
    TRY(check_extent(B, N, "ins_seg_decode"));
    TRY(check_bcn(pts, "pts"));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == DAL3_F32)
        HIP_TRY(launch_ins_seg_decode(view(packed, ins_seg_walk), to_bcn(pts), c_in, B, N,
                                      gbias, logits, mask, s));
    else if (dtype == DAL3_F16X3)
        HIP_TRY(launch_ins_seg_decode_x3(view(packed, ins_seg_16_walk<InsSegX3W>), to_bcn(pts), c_in, B, N, gbias, logits, mask, s));
    else
        HIP_TRY(launch_ins_seg_decode_lp(dtype, view(packed, ins_seg_16_walk<InsSegLpW>), to_bcn(pts), c_in, B, N, gbias, logits, mask, s));
    return 0;
}

// ---------------------------------------------------------------------------------- gather
extern "C" size_t dal3_gather_workspace_bytes(int B, int N) {
    Carver c(nullptr, 0);
    c.take<int32_t>((size_t)B * N);
    return c.off;
}

extern "C" int dal3_segment_counts(const uint8_t* mask, int B, int N, int32_t* counts, dal3_stream stream) {
    if (!mask || !counts) return fail(DAL3_EINVAL, "segment_counts: bad argument");
    TRY(check_extent(B, N, "segment_counts"));
    HIP_TRY(launch_segment_counts(mask, B, N, counts, static_cast<hipStream_t>(stream)));
    return 0;
}

static int gather_run(const uint8_t* mask, const dal3_bcn& pts, int B, int N, int C, int M, int sampler,
                      const int32_t* choice, uint64_t seed, int64_t item_offset, int32_t* counts, int32_t* obj_idx,
                      float* obj_pts, int32_t* pos, hipStream_t s, const int64_t* step = nullptr) {
    if (!mask || !counts || !obj_idx || !obj_pts) return fail(DAL3_EINVAL, "gather: null pointer");
    if (M <= 0 || C <= 0 || C > 8) return fail(DAL3_EINVAL, "gather: bad shape");
    TRY(check_extent(B, N, "gather"));
    TRY(check_extent(B, M, "gather (object points)"));
    if (sampler == DAL3_SAMPLER_CHOICE && !choice) return fail(DAL3_EINVAL, "gather: DAL3_SAMPLER_CHOICE needs choice");
    if (sampler != DAL3_SAMPLER_CHOICE && sampler != DAL3_SAMPLER_DEVICE) return fail(DAL3_EINVAL, "gather: bad sampler");
    TRY(check_bcn(pts, "pts"));
    HIP_TRY(launch_compact_sample(mask, to_bcn(pts), B, N, C, M, sampler, choice, seed, item_offset, counts, pos,
                                  obj_idx, obj_pts, s, step));
    return 0;
}

extern "C" int dal3_mask_compact_sample(const uint8_t* mask, dal3_bcn pts, int B, int N, int C, int M, int sampler,
                                        const int32_t* choice, uint64_t seed, int64_t item_offset, int32_t* counts,
                                        int32_t* obj_idx, float* obj_pts, void* workspace, size_t workspace_bytes,
                                        dal3_stream stream) {
    if (!workspace) return fail(DAL3_EINVAL, "gather: workspace is NULL");
    TRY(check_extent(B, N, "gather"));
    Carver c(workspace, workspace_bytes);
    int32_t* pos = c.take<int32_t>((size_t)B * N);
    if (!c.ok) return fail(DAL3_EWORKSPACE, "gather: workspace needs %zu bytes, got %zu", c.off, workspace_bytes);
    return gather_run(mask, pts, B, N, C, M, sampler, choice, seed, item_offset, counts, obj_idx, obj_pts, pos,
                      static_cast<hipStream_t>(stream));
}

extern "C" int dal3_mask_compact_sample_step(const uint8_t* mask, dal3_bcn pts, int B, int N, int C, int M, uint64_t seed,
                                             const int64_t* step, int64_t item_offset, int32_t* counts, int32_t* obj_idx,
                                             float* obj_pts, void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!workspace) return fail(DAL3_EINVAL, "gather: workspace is NULL");
    TRY(check_extent(B, N, "gather"));
    Carver c(workspace, workspace_bytes);
    int32_t* pos = c.take<int32_t>((size_t)B * N);
    if (!c.ok) return fail(DAL3_EWORKSPACE, "gather: workspace needs %zu bytes, got %zu", c.off, workspace_bytes);
    return gather_run(mask, pts, B, N, C, M, DAL3_SAMPLER_DEVICE, nullptr, seed, item_offset, counts, obj_idx, obj_pts, pos,
                      static_cast<hipStream_t>(stream), step);
}

// ---------------------------------------------------------------------------------- point heads
// `work`: the live-tile worklist of the point heads' persistent kernel (dal3_pointmlp.hip), sized for items of up to
// HEAD_WORK_MAX_POINTS points (the dynamic head's 5 x 512 object points); longer items take the per-tile kernel
#define HEAD_WORK_MAX_POINTS 2560
struct HeadWs { float* feat; float* t1; float* t2; void* work; size_t work_bytes; };
static HeadWs carve_head(Carver& c, int B) {
    HeadWs w;
    w.feat = c.take<float>((size_t)B * 512);
    w.t1 = c.take<float>((size_t)B * 512);
    w.t2 = c.take<float>((size_t)B * 512);
    w.work_bytes = point_head_worklist_bytes(B, HEAD_WORK_MAX_POINTS);
    w.work = c.take<char>(w.work_bytes);
    return w;
}
extern "C" size_t dal3_point_head_workspace_bytes(int B) {
    Carver c(nullptr, 0);
    carve_head(c, B);
    return c.off;
}

// dec (optional): the chain ends in a box estimator's 39-wide layer written to dec->box_pred (= out, row stride 39), and
// that layer is launched together with the decode of its rows (fc39_decode_kernel) instead of on its own
static int fc_chain(const FcW& f, const float* x, int64_t xs, float* out, int64_t out_stride, int B, float* t1,
                    float* t2, hipStream_t s, const DecodeArgs* dec = nullptr) {
    const float* cur = x;
    int64_t cs = xs;
    for (int i = 0; i < f.n; ++i) {
        const bool last = i == f.n - 1;
        float* dst = last ? out : (i % 2 == 0 ? t1 : t2);
        const int64_t ds = last ? out_stride : f.c_out[i];
        if (last && dec) {
            if (f.c_out[i] != 39 || out_stride != 39 || dec->box_pred != out || f.relu[i])
                return fail(DAL3_EINVAL, "fc_chain: a fused decode needs the 39-wide box_pred layer last");
            HIP_TRY(launch_fc39_decode(f.w[i], f.b[i], cur, cs, B, f.c_in[i], *dec, s));
            return 0;
        }
        HIP_TRY(launch_fc(f.w[i], f.b[i], cur, cs, dst, ds, B, f.c_in[i], f.c_out[i], f.relu[i], s));
        cur = dst;
        cs = ds;
    }
    return 0;
}

static int point_head_run(int head_kind, const void* packed, int dtype, const dal3_bcn& x, int B, int M, float* out,
                          int64_t out_stride, const HeadWs& ws, hipStream_t s, const int32_t* distinct = nullptr,
                          const DecodeArgs* dec = nullptr) {
    TRY(check_dtype(dtype));
    if (head_kind != DAL3_HEAD_STATIC_BOX_EST && head_kind != DAL3_HEAD_POINT_EMB && head_kind != DAL3_HEAD_BOX_EMB)
        return fail(DAL3_EINVAL, "point_head: head_kind %d is not a point head", head_kind);
    if (!packed || !out) return fail(DAL3_EINVAL, "point_head: null pointer");
    TRY(check_extent(B, M, "point_head"));
    TRY(check_bcn(x, "x"));
    int c_in, ks, c[4], n_fc, fi[3], fo[3];
    point_head_dims(head_kind, &c_in, &ks, c, &n_fc, fi, fo);
    if (dtype == DAL3_F16X3) {
        const PointHeadX3W w = view(packed, point_head_16_walk, head_kind, true);
        HIP_TRY(launch_point_head_x3(head_kind, w, to_bcn(x), c_in, B, M, ws.feat, distinct, s));
        return fc_chain(w.fc, ws.feat, 512, out, out_stride, B, ws.t1, ws.t2, s, dec);
    }
    if (dtype != DAL3_F32) {
        const PointHeadLpW w = view(packed, point_head_16_walk, head_kind, false);
        HIP_TRY(launch_point_head_lp(dtype, head_kind, w, to_bcn(x), c_in, B, M, ws.feat, distinct, s));
        return fc_chain(w.fc, ws.feat, 512, out, out_stride, B, ws.t1, ws.t2, s, dec);
    }
    const PointHeadW w = view(packed, point_head_walk, head_kind);
    HIP_TRY(launch_point_head(head_kind, w, to_bcn(x), c_in, B, M, ws.feat, distinct, s, ws.work, ws.work_bytes));
    return fc_chain(w.fc, ws.feat, 512, out, out_stride, B, ws.t1, ws.t2, s, dec);
}

extern "C" int dal3_point_head_forward(int head_kind, const void* packed, int dtype, dal3_bcn x, int B, int M, float* out,
                                       int64_t out_stride, void* workspace, size_t workspace_bytes,
                                       dal3_stream stream) {
    if (!workspace) return fail(DAL3_EINVAL, "point_head: workspace is NULL");
    TRY(check_extent(B, M, "point_head"));
    Carver c(workspace, workspace_bytes);
    const HeadWs ws = carve_head(c, B);
    if (!c.ok) return fail(DAL3_EWORKSPACE, "point_head: workspace needs %zu bytes, got %zu", c.off, workspace_bytes);
    return point_head_run(head_kind, packed, dtype, x, B, M, out, out_stride, ws, static_cast<hipStream_t>(stream));
}

/* the per-point stack + max of a point head alone (no FC tail): feat (B,512). n_distinct: see dal3.h */
extern "C" size_t dal3_point_head_pool_workspace_bytes(int B, int M) {
    return B > 0 && M > 0 ? point_head_worklist_bytes(B, M) : 0;
}

extern "C" int dal3_point_head_pool(int head_kind, const void* packed, int dtype, dal3_bcn x, int B, int M,
                                    const int32_t* n_distinct, float* feat, void* workspace, size_t workspace_bytes,
                                    dal3_stream stream) {
    TRY(check_dtype(dtype));
    if (head_kind != DAL3_HEAD_STATIC_BOX_EST && head_kind != DAL3_HEAD_POINT_EMB && head_kind != DAL3_HEAD_BOX_EMB)
        return fail(DAL3_EINVAL, "point_head_pool: head_kind %d is not a point head", head_kind);
    if (!packed || !feat) return fail(DAL3_EINVAL, "point_head_pool: null pointer");
    if (workspace && (reinterpret_cast<uintptr_t>(workspace) & 15)) return fail(DAL3_EINVAL, "point_head_pool: workspace must be 16-byte aligned");
    TRY(check_extent(B, M, "point_head_pool"));
    TRY(check_bcn(x, "x"));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int c_in, ks, c[4], n_fc, fi[3], fo[3];
    point_head_dims(head_kind, &c_in, &ks, c, &n_fc, fi, fo);
    if (dtype == DAL3_F16X3) {
        HIP_TRY(launch_point_head_x3(head_kind, view(packed, point_head_16_walk, head_kind, true), to_bcn(x), c_in, B, M, feat, n_distinct, s));
        return 0;
    }
    if (dtype != DAL3_F32) {
        const PointHeadLpW w = view(packed, point_head_16_walk, head_kind, false);
        HIP_TRY(launch_point_head_lp(dtype, head_kind, w, to_bcn(x), c_in, B, M, feat, n_distinct, s));
        return 0;
    }
    const PointHeadW w = view(packed, point_head_walk, head_kind);
    HIP_TRY(launch_point_head(head_kind, w, to_bcn(x), c_in, B, M, feat, n_distinct, s, workspace, workspace_bytes));
    return 0;
}

extern "C" int dal3_point_head_screen_min_tiles(void) { return DAL3_HEAD_SCREEN ? DAL3_HEAD_SCR_MIN_TILES : 0x7fffffff; }
extern "C" int dal3_point_head_screen_stride(void) { return DAL3_HEAD_SCR_STRIDE; }
extern "C" int dal3_point_head_route(int head_kind, int B, int M, int flags) {
    TRY(check_extent(B, M, "point_head_route"));
    if (head_kind < 1 || head_kind > 3) return fail(DAL3_EINVAL, "point_head_route: unknown head kind %d", head_kind);
    if (flags & ~(DAL3_BCN_NO_SMALL_JOB_KERNELS | DAL3_BCN_NO_WORKLIST | DAL3_BCN_NO_LDS_SAMPLER | DAL3_BCN_NO_DEC_PLAN | DAL3_BCN_NO_ENC_RESIDENT | DAL3_BCN_NO_HEAD_RESIDENT | DAL3_BCN_NO_DEC_PAIR))
        return fail(DAL3_EINVAL, "point_head_route: unknown bits in flags (%d)", flags);
    return head_route(flags, head_kind, B, M);
}

extern "C" int dal3_dynamic_box_est_forward(const void* packed, const float* embedding, int B, float* box_pred,
                                            void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!packed || !embedding || !box_pred || !workspace) return fail(DAL3_EINVAL, "dynamic_box_est: bad argument");
    TRY(check_extent(B, 1, "dynamic_box_est"));
    Carver c(workspace, workspace_bytes);
    const HeadWs ws = carve_head(c, B);
    if (!c.ok) return fail(DAL3_EWORKSPACE, "dynamic_box_est: workspace needs %zu bytes, got %zu", c.off, workspace_bytes);
    return fc_chain(view(packed, fc_head_walk), embedding, 384, box_pred, 39, B, ws.t1, ws.t2,
                    static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------------- small entries
extern "C" int dal3_decode_boxes(float* box_pred, int B, const float* center_add, int64_t center_add_stride,
                                 int center_inplace, const float* boxes_center_add, int64_t boxes_center_add_stride,
                                 const float* yaw_base, int64_t yaw_stride, float* heading_residuals,
                                 float* size_residuals, float* center, float* boxes7, dal3_stream stream) {
    if (!box_pred || B <= 0) return fail(DAL3_EINVAL, "decode_boxes: bad argument");
    HIP_TRY(launch_decode_boxes(box_pred, B, center_add, center_add_stride, center_inplace, boxes_center_add,
                                boxes_center_add_stride, yaw_base, yaw_stride, heading_residuals, size_residuals,
                                center, boxes7, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_recenter_rotz(const float* obj_pts, int B, int M, const float* init_box7, const float* box_one7,
                                  const float* bbox_gt7, float* obj_pts_two, int64_t* heading_class_label,
                                  float* heading_residual_label, dal3_stream stream) {
    if (!obj_pts || !init_box7 || !box_one7 || !obj_pts_two || B <= 0 || M <= 0)
        return fail(DAL3_EINVAL, "recenter_rotz: bad argument");
    if (bbox_gt7 && (!heading_class_label || !heading_residual_label))
        return fail(DAL3_EINVAL, "recenter_rotz: bbox_gt given without label outputs");
    HIP_TRY(launch_recenter(obj_pts, B, M, init_box7, box_one7, bbox_gt7, obj_pts_two, heading_class_label,
                            heading_residual_label, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_static_crop_prep(const double* points, const int64_t* offsets, const int32_t* choice,
                                     const double* pose, const double* box, int B, int N, uint64_t seed,
                                     int64_t item_offset, float* pts_out, float* init_box_out, dal3_stream stream) {
    if (!points || !offsets || !pose || !box || !pts_out || !init_box_out || B <= 0 || N < 7)
        return fail(DAL3_EINVAL, "static_crop_prep: bad argument (N must be >= 7)");
    HIP_TRY(launch_static_crop_prep(points, offsets, choice, pose, box, B, N, seed, item_offset, pts_out, init_box_out,
                                    static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_dynamic_item_prep(const double* points, const int64_t* frame_offsets, const double* boxes,
                                      const int64_t* track_first, const int32_t* item_track, const int32_t* item_frame,
                                      const int32_t* choice, const double* pose, int B, int n_per, int r, int s,
                                      uint64_t seed, int64_t item_offset, float* pts_out, float* box_out,
                                      float* init_box_out, dal3_stream stream) {
    if (!points || !frame_offsets || !boxes || !track_first || !item_track || !item_frame || !pose || !pts_out ||
        !box_out || !init_box_out || B <= 0 || n_per <= 0 || r < 0 || s < 0)
        return fail(DAL3_EINVAL, "dynamic_item_prep: bad argument");
    HIP_TRY(launch_dynamic_item_prep(points, frame_offsets, boxes, track_first, item_track, item_frame, choice, pose, B,
                                     n_per, r, s, seed, item_offset, pts_out, box_out, init_box_out,
                                     static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_static_crop_labels(const double* points, const int64_t* offsets, const int32_t* choice,
                                       const double* pose, int B, int N, uint64_t seed, int64_t item_offset,
                                       const double* gt_planes, uint8_t* mask_label, dal3_stream stream) {
    if (!points || !offsets || !pose || !gt_planes || !mask_label || B <= 0 || N <= 0)
        return fail(DAL3_EINVAL, "static_crop_labels: bad argument");
    HIP_TRY(launch_static_crop_labels(points, offsets, choice, pose, B, N, seed, item_offset, gt_planes, mask_label,
                                      static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_dynamic_item_labels(const double* points, const int64_t* frame_offsets, const int64_t* track_first,
                                        const int32_t* item_track, const int32_t* item_frame, const int32_t* choice,
                                        const double* pose, int B, int n_per, int r, uint64_t seed, int64_t item_offset,
                                        const double* xform, const double* planes, const uint8_t* valid,
                                        uint8_t* mask_label, dal3_stream stream) {
    if (!points || !frame_offsets || !track_first || !item_track || !item_frame || !pose || !xform || !planes || !valid ||
        !mask_label || B <= 0 || n_per <= 0 || r < 0)
        return fail(DAL3_EINVAL, "dynamic_item_labels: bad argument");
    HIP_TRY(launch_dynamic_item_labels(points, frame_offsets, track_first, item_track, item_frame, choice, pose, B, n_per, r,
                                       seed, item_offset, xform, planes, valid, mask_label,
                                       static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_points_in_boxes(const void* points, int points_f64, int64_t P, int64_t stride, const double* planes,
                                    int K, int f32_math, uint8_t* inside, dal3_stream stream) {
    if (P < 0 || K < 0 || stride < 3 || ((P > 0 && K > 0) && (!points || !planes || !inside)))
        return fail(DAL3_EINVAL, "points_in_boxes: bad argument (stride must be >= 3)");
    if (points_f64 && f32_math) return fail(DAL3_EINVAL, "points_in_boxes: float32 arithmetic needs float32 points");
    HIP_TRY(launch_points_in_boxes(points, points_f64, P, stride, planes, K, f32_math, inside,
                                   static_cast<hipStream_t>(stream)));
    return 0;
}

static int box_iou_args_ok(const char* what, const void* a, int64_t n, const void* b, int64_t m, int boxes_f64,
                           const float* iou_bev, const float* iou_3d, int64_t blocks) {
    if (n < 0 || m < 0 || (boxes_f64 != 0 && boxes_f64 != 1))
        return fail(DAL3_EINVAL, "%s: bad argument (n, m >= 0, boxes_f64 0 or 1)", what);
    if (n > DAL3_MAX_ITEMS || m > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "%s: more than DAL3_MAX_ITEMS boxes on one side; split the call", what);
    if (blocks > DAL3_MAX_TILES) return fail(DAL3_EINVAL, "%s: launch grid beyond DAL3_MAX_TILES; split the call", what);
    if (!iou_bev && !iou_3d) return fail(DAL3_EINVAL, "%s: no output (iou_bev and iou_3d both NULL)", what);
    if (n > 0 && m > 0 && (!a || !b)) return fail(DAL3_EINVAL, "%s: null boxes", what);
    return 0;
}

extern "C" int dal3_box_iou_pairwise(const void* a, int64_t n, const void* b, int64_t m, int boxes_f64, float* iou_bev,
                                     float* iou_3d, dal3_stream stream) {
    // the block count is formed only once n, m are known to be <= 2^24 each: n * m / 1024 < 2^38, no overflow
    const int64_t blocks = (n >= 0 && m >= 0 && n <= DAL3_MAX_ITEMS && m <= DAL3_MAX_ITEMS) ? box_iou_pairwise_blocks(n, m) : 0;
    TRY(box_iou_args_ok("box_iou_pairwise", a, n, b, m, boxes_f64, iou_bev, iou_3d, blocks));
    HIP_TRY(launch_box_iou_pairwise(a, n, b, m, boxes_f64, iou_bev, iou_3d, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_box_iou_paired(const void* a, const void* b, int64_t n, int boxes_f64, float* iou_bev, float* iou_3d,
                                   dal3_stream stream) {
    const int64_t blocks = (n >= 0 && n <= DAL3_MAX_ITEMS) ? box_iou_paired_blocks(n) : 0;
    TRY(box_iou_args_ok("box_iou_paired", a, n, b, n, boxes_f64, iou_bev, iou_3d, blocks));
    HIP_TRY(launch_box_iou_paired(a, b, n, boxes_f64, iou_bev, iou_3d, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_box_estimation_metrics(const dal3_box_metric_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "box_estimation_metrics: null args");
    const dal3_box_metric_args& a = *args;
    if (a.B < 0 || a.N < 0 || a.B > DAL3_MAX_ITEMS || a.N > DAL3_MAX_POINTS_PER_ITEM)
        return fail(DAL3_EINVAL, "box_estimation_metrics: bad B / N (0 <= B <= DAL3_MAX_ITEMS, 0 <= N <= DAL3_MAX_POINTS_PER_ITEM)");
    if (!a.acc && !a.iou_bev && !a.iou_3d) return fail(DAL3_EINVAL, "box_estimation_metrics: no accumulator and no output");
    if ((a.f64_fields & ~255) || (a.i32_fields & ~3))
        return fail(DAL3_EINVAL, "box_estimation_metrics: unknown bits in f64_fields / i32_fields");
    if (a.B > 0) {
        const void* need[10] = {a.center, a.heading_scores, a.heading_residuals, a.size_scores, a.size_residuals,
                                a.center_label, a.heading_class_label, a.heading_residual_label, a.size_class_label,
                                a.size_residual_label};
        const int64_t ld[10] = {a.ld_center, a.ld_heading_scores, a.ld_heading_residuals, a.ld_size_scores,
                                a.ld_size_residuals, a.ld_center_label, a.ld_heading_class_label,
                                a.ld_heading_residual_label, a.ld_size_class_label, a.ld_size_residual_label};
        for (int k = 0; k < 10; ++k) {
            if (!need[k]) return fail(DAL3_EINVAL, "box_estimation_metrics: null field %d", k);
            if (ld[k] < 0) return fail(DAL3_EINVAL, "box_estimation_metrics: negative row stride of field %d", k);
        }
    }
    if (a.logits) {
        if (!a.acc) return fail(DAL3_EINVAL, "box_estimation_metrics: the segmentation term needs the accumulator");
        if (a.B > 0 && a.N > 0 && !a.mask_label) return fail(DAL3_EINVAL, "box_estimation_metrics: null mask_label");
        if (a.mask_dtype != DAL3_MASK_U8 && a.mask_dtype != DAL3_MASK_F32)
            return fail(DAL3_EINVAL, "box_estimation_metrics: mask_dtype must be DAL3_MASK_U8 or DAL3_MASK_F32");
        if (a.logits_stride_b < 0 || a.logits_stride_n < 0 || a.logits_stride_c < 0 || a.mask_stride_b < 0 ||
            a.mask_stride_n < 0)
            return fail(DAL3_EINVAL, "box_estimation_metrics: negative stride");
        if (1 + a.B * box_estimation_metrics_chunks(a.N) > DAL3_MAX_TILES)
            return fail(DAL3_EINVAL, "box_estimation_metrics: launch grid beyond DAL3_MAX_TILES; split the call");
    }
    HIP_TRY(launch_box_estimation_metrics(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_track_workspace_bytes(int64_t S, int64_t K, int64_t capacity) {
    if (S < 0 || K < 0 || capacity < 1 || capacity > DAL3_TRACK_MAX_CAPACITY) return 0;
    return track_workspace_bytes(S, K, capacity);
}

extern "C" int dal3_track(const dal3_track_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "track: null args");
    const dal3_track_args& a = *args;
    if (a.S < 0 || a.F < 0 || a.K < 0 || a.K > DAL3_MAX_ITEMS || a.F > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "track: bad S / F / K (0 <= F, K <= DAL3_MAX_ITEMS)");
    if (a.capacity < 1 || a.capacity > DAL3_TRACK_MAX_CAPACITY)
        return fail(DAL3_EINVAL, "track: capacity must be in [1, DAL3_TRACK_MAX_CAPACITY]");
    if (a.max_workgroups < 0) return fail(DAL3_EINVAL, "track: negative max_workgroups");
    if (!a.seq_offsets || !a.frame_offsets || !a.status || !a.workspace)
        return fail(DAL3_EINVAL, "track: null offsets / status / workspace");
    if (a.F > 0 && !a.out_count) return fail(DAL3_EINVAL, "track: null out_count");
    if (a.K > 0 && (!a.ct || !a.tracking || !a.label || !a.score || !a.box_ids || !a.tracking_ids))
        return fail(DAL3_EINVAL, "track: null detection input / output");
    if (a.workspace_bytes < track_workspace_bytes(a.S, a.K, a.capacity))
        return fail(DAL3_EWORKSPACE, "track: workspace too small (dal3_track_workspace_bytes)");
    HIP_TRY(launch_track(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_track_match_workspace_bytes(int64_t K) {
    if (K < 0) return 0;
    return track_match_workspace_bytes(K);
}

extern "C" int dal3_track_match(const dal3_track_match_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "track_match: null args");
    const dal3_track_match_args& a = *args;
    if (a.F < 0 || a.K < 0 || a.K > DAL3_MAX_ITEMS || a.F > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "track_match: bad F / K (0 <= F, K <= DAL3_MAX_ITEMS)");
    if (a.K > 0 && a.F > 0 && (!a.frame_offsets || !a.out_count || !a.box_ids || !a.tracking_ids || !a.boxes ||
                               !a.gt_offsets || !a.match_frame || !a.match_obj || !a.status || !a.workspace))
        return fail(DAL3_EINVAL, "track_match: null argument");
    if (a.workspace_bytes < track_match_workspace_bytes(a.K))
        return fail(DAL3_EWORKSPACE, "track_match: workspace too small (dal3_track_match_workspace_bytes)");
    HIP_TRY(launch_track_match(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_group_workspace_bytes(int64_t E, int64_t T) {
    if (E < 0 || T < 0 || E > DAL3_MAX_ITEMS || T > DAL3_MAX_ITEMS) return 0;
    return group_workspace_bytes(E, T);
}

extern "C" int dal3_group_by_key(const dal3_group_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "group_by_key: null args");
    const dal3_group_args& a = *args;
    if (a.E < 0 || a.T < 0 || a.F < 0 || a.E > DAL3_MAX_ITEMS || a.T > DAL3_MAX_ITEMS || a.F > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "group_by_key: bad E / T / F (0 <= E, T, F <= DAL3_MAX_ITEMS)");
    if (a.max_workgroups < 0) return fail(DAL3_EINVAL, "group_by_key: negative max_workgroups");
    if (!a.group_start || !a.status) return fail(DAL3_EINVAL, "group_by_key: null group_start / status");
    if (a.E > 0 && (!a.keys || !a.entry || !a.workspace)) return fail(DAL3_EINVAL, "group_by_key: null keys / entry / workspace");
    if ((a.frame_offsets == nullptr) != (a.out_count == nullptr))
        return fail(DAL3_EINVAL, "group_by_key: frame_offsets and out_count go together");
    if (!a.frame_offsets && a.F != 0) return fail(DAL3_EINVAL, "group_by_key: F without frame_offsets");
    if (a.workspace_bytes < group_workspace_bytes(a.E, a.T))
        return fail(DAL3_EWORKSPACE, "group_by_key: workspace too small (dal3_group_workspace_bytes)");
    HIP_TRY(launch_group_by_key(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_track_features(const dal3_track_feature_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "track_features: null args");
    const dal3_track_feature_args& a = *args;
    if (a.T < 0 || a.E < 0 || a.E > DAL3_MAX_ITEMS || a.T > DAL3_MAX_ITEMS || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "track_features: bad T / E / max_workgroups");
    if (a.T > 0 && (!a.group_start || !a.n || !a.type0 || !a.match_last || !a.points_sum || !a.best || !a.keep || !a.feature))
        return fail(DAL3_EINVAL, "track_features: null group_start / output");
    if (a.T > 0 && a.E > 0 && (!a.entry || !a.center || !a.type || !a.score || !a.n_points || !a.match))
        return fail(DAL3_EINVAL, "track_features: null per-entry input");
    HIP_TRY(launch_track_features(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_gt_table(const dal3_gt_table_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "gt_table: null args");
    const dal3_gt_table_args& a = *args;
    if (a.T < 0 || a.E < 0 || a.F < 0 || a.E > DAL3_MAX_ITEMS || a.T > DAL3_MAX_ITEMS || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "gt_table: bad T / E / F / max_workgroups");
    if (!a.status) return fail(DAL3_EINVAL, "gt_table: null status");
    if (a.T > 0 && (!a.group_start || !a.n || !a.dist || !a.max_vel || !a.is_static))
        return fail(DAL3_EINVAL, "gt_table: null group_start / output");
    if (a.E > 0 && (!a.entry || !a.box || !a.frame || !a.box_global || !a.vel || (a.F > 0 && !a.pose)))
        return fail(DAL3_EINVAL, "gt_table: null per-entry argument");
    HIP_TRY(launch_gt_table(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_motion_classify_workspace_bytes(int64_t T) {
    if (T < 0 || T > DAL3_MAX_ITEMS) return 0;
    return motion_classify_workspace_bytes(T);
}

extern "C" int dal3_motion_classify(const dal3_motion_classify_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "motion_classify: null args");
    const dal3_motion_classify_args& a = *args;
    if (a.T < 0 || a.T > DAL3_MAX_ITEMS || a.max_workgroups < 0) return fail(DAL3_EINVAL, "motion_classify: bad T / max_workgroups");
    if (!a.counts || !a.workspace) return fail(DAL3_EINVAL, "motion_classify: null counts / workspace");
    if (a.T > 0 && (!a.feature || !a.keep || !a.decision || !a.is_static || !a.static_ids || !a.dynamic_ids))
        return fail(DAL3_EINVAL, "motion_classify: null argument");
    if (a.workspace_bytes < motion_classify_workspace_bytes(a.T))
        return fail(DAL3_EWORKSPACE, "motion_classify: workspace too small (dal3_motion_classify_workspace_bytes)");
    HIP_TRY(launch_motion_classify(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_score_workspace_bytes(int64_t S) {
    if (S < 0 || S > DAL3_MAX_ITEMS) return 0;
    return score_workspace_bytes(S);
}

extern "C" int dal3_score_tracks(const dal3_score_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "score_tracks: null args");
    const dal3_score_args& a = *args;
    if (a.S < 0 || a.R < 0 || a.F < 0 || a.S > DAL3_MAX_ITEMS || a.R > DAL3_MAX_ITEMS || a.F > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "score_tracks: bad S / R / F (0 <= S, R, F <= DAL3_MAX_ITEMS)");
    if ((a.gt_f64 != 0 && a.gt_f64 != 1) || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "score_tracks: bad argument (gt_f64 0 or 1, max_workgroups >= 0)");
    if (!a.acc && !a.iou_bev && !a.iou_3d && !a.pred_box && !a.label_box)
        return fail(DAL3_EINVAL, "score_tracks: no accumulator and no output");
    if (a.S == 0) return 0;                                 // nothing to score: acc stays as it is
    if (!a.box_row || !a.frame || !a.has_gt || !a.type) return fail(DAL3_EINVAL, "score_tracks: null per-sample table");
    if ((a.R > 0 && !a.boxes) || (a.F > 0 && !a.pose_inv) || !a.gt) return fail(DAL3_EINVAL, "score_tracks: null boxes / pose_inv / gt");
    if (a.acc) {
        if (!a.workspace) return fail(DAL3_EINVAL, "score_tracks: the accumulator needs a workspace");
        if (a.workspace_bytes < score_workspace_bytes(a.S))
            return fail(DAL3_EWORKSPACE, "score_tracks: workspace too small (dal3_score_workspace_bytes)");
        if (reinterpret_cast<uintptr_t>(a.workspace) & 7) return fail(DAL3_EINVAL, "score_tracks: workspace must be 8-byte aligned");
    }
    HIP_TRY(launch_score_tracks(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_best_gt_iou(const dal3_best_gt_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "best_gt_iou: null args");
    const dal3_best_gt_args& a = *args;
    if (a.Q < 0 || a.F < 0 || a.G < 0 || a.Q > DAL3_MAX_ITEMS || a.F > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "best_gt_iou: bad Q / F / G (0 <= Q, F <= DAL3_MAX_ITEMS, G >= 0)");
    if ((a.boxes_f64 != 0 && a.boxes_f64 != 1) || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "best_gt_iou: bad argument (boxes_f64 0 or 1, max_workgroups >= 0)");
    if (a.Q == 0) return 0;
    if (!a.best_iou_3d) return fail(DAL3_EINVAL, "best_gt_iou: no output (best_iou_3d is NULL)");
    if (!a.queries || !a.query_frame || (a.F > 0 && !a.gt_offsets) || (a.G > 0 && !a.gt_boxes))
        return fail(DAL3_EINVAL, "best_gt_iou: null queries / query_frame / gt_offsets / gt_boxes");
    HIP_TRY(launch_best_gt_iou(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_nms_workspace_bytes(int64_t K, int boxes_f64) {
    if (K < 0 || K > DAL3_MAX_ITEMS || (boxes_f64 != 0 && boxes_f64 != 1)) return 0;
    return nms_workspace_bytes(K, boxes_f64);
}

extern "C" int dal3_nms(const dal3_nms_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "nms: null args");
    const dal3_nms_args& a = *args;
    if (a.F < 0 || a.K < 0 || a.F > DAL3_MAX_ITEMS || a.K > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "nms: bad F / K (0 <= F, K <= DAL3_MAX_ITEMS)");
    if (a.mode != DAL3_NMS_ROTATE && a.mode != DAL3_NMS_CIRCLE) return fail(DAL3_EINVAL, "nms: unknown mode %d", (int)a.mode);
    if ((a.boxes_f64 != 0 && a.boxes_f64 != 1) || (a.mirror != 0 && a.mirror != 1) || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "nms: bad argument (boxes_f64 0 or 1, mirror 0 or 1, max_workgroups >= 0)");
    if (a.box_stride < 7 || a.yaw_col < 6 || a.yaw_col >= a.box_stride)
        return fail(DAL3_EINVAL, "nms: bad box layout (box_stride >= 7, 6 <= yaw_col < box_stride)");
    if (a.pre_max < 0 || a.post_max < 0 || a.stride < 0) return fail(DAL3_EINVAL, "nms: negative pre_max / post_max / stride");
    if (a.pre_max > DAL3_NMS_MAX_PRE) return fail(DAL3_EINVAL, "nms: pre_max above DAL3_NMS_MAX_PRE (%d)", DAL3_NMS_MAX_PRE);
    if (a.thresh != a.thresh) return fail(DAL3_EINVAL, "nms: thresh is NaN");
    if (a.F == 0) return 0;
    if (!a.keep_count || !a.status || !a.seg_offsets || !a.seg_offsets_host)
        return fail(DAL3_EINVAL, "nms: null keep_count / status / seg_offsets / seg_offsets_host");
    int64_t max_n = 0;
    for (int64_t f = 0; f < a.F; ++f) {
        const int64_t d0 = a.seg_offsets_host[f], d1 = a.seg_offsets_host[f + 1];
        if (d0 < 0 || d1 < d0 || d1 > a.K)
            return fail(DAL3_EINVAL, "nms: seg_offsets must be non-decreasing within [0, K] (segment %lld: %lld .. %lld)",
                        (long long)f, (long long)d0, (long long)d1);
        if (d1 - d0 > max_n) max_n = d1 - d0;
    }
    const int64_t need = a.post_max > 0 && a.post_max < max_n ? a.post_max : max_n;
    if (a.stride < need)
        return fail(DAL3_EINVAL, "nms: stride %lld too small (min(post_max or N, N) = %lld)", (long long)a.stride, (long long)need);
    if (a.stride > 0 && !a.keep) return fail(DAL3_EINVAL, "nms: null keep");
    if (a.K > 0 && (!a.boxes || !a.scores || !a.workspace)) return fail(DAL3_EINVAL, "nms: null boxes / scores / workspace");
    if (a.workspace_bytes < nms_workspace_bytes(a.K, a.boxes_f64))
        return fail(DAL3_EWORKSPACE, "nms: workspace too small (dal3_nms_workspace_bytes)");
    if (reinterpret_cast<uintptr_t>(a.workspace) & 7) return fail(DAL3_EINVAL, "nms: workspace must be 8-byte aligned");
    HIP_TRY(launch_nms(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_center_decode_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    if (B < 0 || H < 0 || W < 0 || B > DAL3_MAX_ITEMS || H > DAL3_MAX_ITEMS || W > DAL3_MAX_ITEMS || H * W > DAL3_MAX_ITEMS)
        return 0;
    return center_decode_workspace_bytes(B, H, W);
}

// the checks dal3_center_decode and dal3_center_decode_flip4 share (B: the samples that are written)
static int check_center_decode(const dal3_center_decode_args& a, const char* who) {
    if (a.B < 0 || a.H <= 0 || a.W <= 0 || a.B > DAL3_MAX_ITEMS || a.H > DAL3_MAX_ITEMS || a.W > DAL3_MAX_ITEMS ||
        a.H * a.W > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "%s: bad B / H / W (H, W >= 1, B, H W <= DAL3_MAX_ITEMS)", who);
    if (a.C < 1 || a.C > 64) return fail(DAL3_EINVAL, "%s: bad C (1 <= C <= 64)", who);
    if (a.F < 0 || a.K < 0 || a.F > DAL3_MAX_ITEMS || a.K > DAL3_MAX_ITEMS || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "%s: bad F / K / max_workgroups", who);
    if (a.B == 0) return 0;
    const int64_t last = a.seg_first + (a.B - 1) * a.seg_step;
    if (a.seg_first < 0 || a.seg_first >= a.F || last < 0 || last >= a.F || (a.B > 1 && a.seg_step == 0))
        return fail(DAL3_EINVAL, "%s: segments seg_first + b * seg_step must be distinct and lie in [0, F)", who);
    if (!a.hm.data || !a.reg.data || !a.height.data || !a.dim.data || !a.rot.data)
        return fail(DAL3_EINVAL, "%s: null hm / reg / height / dim / rot", who);
    if (!a.seg_offsets || !a.seg_count || !a.status || !a.workspace)
        return fail(DAL3_EINVAL, "%s: null seg_offsets / seg_count / status / workspace", who);
    if (a.K > 0 && (!a.boxes || !a.scores || !a.labels || !a.cell))
        return fail(DAL3_EINVAL, "%s: null boxes / scores / labels / cell", who);
    if (a.workspace_bytes < center_decode_workspace_bytes(a.B, a.H, a.W))
        return fail(DAL3_EWORKSPACE, "%s: workspace too small (dal3_%s_workspace_bytes)", who, who);
    return 0;
}

extern "C" int dal3_center_decode(const dal3_center_decode_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "center_decode: null args");
    TRY(check_center_decode(*args, "center_decode"));
    if (args->B == 0) return 0;
    HIP_TRY(launch_center_decode(args, static_cast<hipStream_t>(stream)));
    return 0;
}

// the merged samples share dal3_center_decode's chunks, so its workspace
extern "C" size_t dal3_center_decode_flip4_workspace_bytes(int64_t B, int64_t H, int64_t W) {
    return dal3_center_decode_workspace_bytes(B, H, W);
}

extern "C" int dal3_center_decode_flip4(const dal3_center_decode_flip4_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "center_decode_flip4: null args");
    if (args->decode.B > DAL3_MAX_ITEMS / 4)
        return fail(DAL3_EINVAL, "center_decode_flip4: bad B (the maps hold 4 B <= DAL3_MAX_ITEMS samples)");
    TRY(check_center_decode(args->decode, "center_decode_flip4"));
    if (args->decode.B == 0) return 0;
    HIP_TRY(launch_center_decode_flip4(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_flip4_points(const float* points, int64_t N, int32_t C, const int64_t* offsets, int64_t B, float* out,
                                 int64_t* out_offsets, int64_t max_workgroups, dal3_stream stream) {
    if (B < 0 || N < 0 || B > DAL3_MAX_ITEMS / 4 || N > DAL3_MAX_ITEMS / 4)
        return fail(DAL3_EINVAL, "flip4_points: bad B / N (0 <= B, N <= DAL3_MAX_ITEMS / 4)");
    if (C < 2 || C > 64) return fail(DAL3_EINVAL, "flip4_points: bad C (2 <= C <= 64)");
    if (max_workgroups < 0) return fail(DAL3_EINVAL, "flip4_points: negative max_workgroups");
    if (B == 0) return 0;
    if (!offsets || !out_offsets) return fail(DAL3_EINVAL, "flip4_points: null offsets / out_offsets");
    if (N > 0 && (!points || !out)) return fail(DAL3_EINVAL, "flip4_points: null points / out");
    HIP_TRY(launch_flip4_points(points, N, C, offsets, B, out, out_offsets, max_workgroups, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_sweep_merge(const dal3_sweep_segment* segments, int64_t B, int32_t nsweeps, int64_t N, float* out,
                                int64_t* point_offsets, int64_t max_workgroups, dal3_stream stream) {
    if (nsweeps < 1 || nsweeps > DAL3_SWEEP_MAX) return fail(DAL3_EINVAL, "sweep_merge: bad nsweeps (1 .. DAL3_SWEEP_MAX)");
    if (B < 0 || N < 0 || B * nsweeps > DAL3_MAX_ITEMS || N > DAL3_MAX_TILES)
        return fail(DAL3_EINVAL, "sweep_merge: bad B / N (0 <= B * nsweeps <= DAL3_MAX_ITEMS, 0 <= N <= DAL3_MAX_TILES)");
    if (max_workgroups < 0) return fail(DAL3_EINVAL, "sweep_merge: negative max_workgroups");
    if (B == 0) return 0;
    if (!segments || !point_offsets) return fail(DAL3_EINVAL, "sweep_merge: null segments / point_offsets");
    if (reinterpret_cast<uintptr_t>(segments) % 8 || reinterpret_cast<uintptr_t>(point_offsets) % 8)
        return fail(DAL3_EINVAL, "sweep_merge: segments and point_offsets must be 8-byte aligned");
    if (N > 0 && (!out || reinterpret_cast<uintptr_t>(out) % 4)) return fail(DAL3_EINVAL, "sweep_merge: null or misaligned out");
    HIP_TRY(launch_sweep_merge(segments, B, nsweeps, N, out, point_offsets, max_workgroups, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---------------------------------------------------------------------------------- the PointPillars reader
extern "C" size_t dal3_voxelize_workspace_bytes(int64_t B, int64_t N) {
    if (B < 0 || N < 0 || B > DAL3_MAX_ITEMS || N > DAL3_MAX_ITEMS) return 0;
    return voxelize_workspace_bytes(B, N);
}

extern "C" int dal3_voxelize(const dal3_voxelize_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "voxelize: null args");
    const dal3_voxelize_args& a = *args;
    if (a.B < 0 || a.N < 0 || a.B > DAL3_MAX_ITEMS || a.N > DAL3_MAX_ITEMS)
        return fail(DAL3_EINVAL, "voxelize: bad B / N (0 <= B, N <= DAL3_MAX_ITEMS)");
    if (a.C < 3 || a.C > 8 || a.point_stride < a.C) return fail(DAL3_EINVAL, "voxelize: bad point layout (3 <= C <= 8, point_stride >= C)");
    if ((a.reverse_index != 0 && a.reverse_index != 1) || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "voxelize: bad argument (reverse_index 0 or 1, max_workgroups >= 0)");
    if (a.max_points < 1 || a.max_points > 65536 || a.max_voxels < 1 || a.capacity < 0)
        return fail(DAL3_EINVAL, "voxelize: bad max_points (1 .. 65536) / max_voxels (>= 1) / capacity (>= 0)");
    for (int j = 0; j < 3; ++j) {
        if (a.grid[j] < 1) return fail(DAL3_EINVAL, "voxelize: grid[%d] = %d, every axis needs a cell", j, (int)a.grid[j]);
        if (!(a.voxel_size[j] > 0.f) || !(a.pc_range[j] - a.pc_range[j] == 0.f) || !(a.voxel_size[j] - a.voxel_size[j] == 0.f))
            return fail(DAL3_EINVAL, "voxelize: voxel_size must be positive and finite, pc_range finite");
    }
    const int64_t cells = (int64_t)a.grid[0] * a.grid[1] * a.grid[2];
    if (a.grid[0] > 65536 || a.grid[1] > 65536 || a.grid[2] > 65536 || cells >= 2147483647 || (a.B > 0 && cells >= 2147483647 / a.B))
        return fail(DAL3_EINVAL, "voxelize: the (sample, cell) key needs B * cells < 2^31 - 1 (split the batch)");
    if (!a.voxel_offsets || !a.status) return fail(DAL3_EINVAL, "voxelize: null voxel_offsets / status");
    if (a.B > 0 && (!a.point_offsets || !a.point_offsets_host))
        return fail(DAL3_EINVAL, "voxelize: null point_offsets / point_offsets_host");
    int64_t need = 0;
    for (int64_t b = 0; b < a.B; ++b) {
        const int64_t d0 = a.point_offsets_host[b], d1 = a.point_offsets_host[b + 1];
        if (d0 < 0 || d1 < d0 || d1 > a.N)
            return fail(DAL3_EINVAL, "voxelize: point_offsets must be non-decreasing within [0, N] (sample %lld: %lld .. %lld)",
                        (long long)b, (long long)d0, (long long)d1);
        int64_t n = d1 - d0;
        if (n > a.max_voxels) n = a.max_voxels;
        if (n > cells) n = cells;
        need += n;
    }
    if (a.capacity < need)
        return fail(DAL3_EINVAL, "voxelize: capacity %lld too small (the samples' min(points, max_voxels, cells) sum to %lld)",
                    (long long)a.capacity, (long long)need);
    if (a.capacity > DAL3_MAX_ITEMS) return fail(DAL3_EINVAL, "voxelize: capacity above DAL3_MAX_ITEMS");
    if (a.capacity > 0 && (!a.voxels || !a.coordinates || !a.num_points))
        return fail(DAL3_EINVAL, "voxelize: null voxels / coordinates / num_points");
    if (a.N > 0 && a.B > 0) {
        if (!a.points || !a.workspace) return fail(DAL3_EINVAL, "voxelize: null points / workspace");
        if (a.workspace_bytes < voxelize_workspace_bytes(a.B, a.N))
            return fail(DAL3_EWORKSPACE, "voxelize: workspace too small (dal3_voxelize_workspace_bytes)");
        if (reinterpret_cast<uintptr_t>(a.workspace) & 7) return fail(DAL3_EINVAL, "voxelize: workspace must be 8-byte aligned");
    }
    HIP_TRY(launch_voxelize(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_pillar_pack(const dal3_layer* layers, int n_layers, int C, double eps, float* out, dal3_stream stream) {
    if (!layers || !out) return fail(DAL3_EINVAL, "pillar_pack: null layers / out");
    if (n_layers != 1 && n_layers != 2) return fail(DAL3_EINVAL, "pillar_pack: %d layers (1 or 2)", n_layers);
    if (C < 3 || C > 8 || !(eps > 0.0)) return fail(DAL3_EINVAL, "pillar_pack: bad C (3 .. 8) / eps (> 0)");
    const int want_in[2] = {C + 5, 64}, want_out[2] = {n_layers == 1 ? 64 : 32, 64};
    for (int i = 0; i < n_layers; ++i) {
        const dal3_layer& L = layers[i];
        if (L.c_in != want_in[i] || L.c_out != want_out[i])
            return fail(DAL3_EINVAL, "pillar_pack: layer %d is %d -> %d, the kernel serves %d -> %d", i, (int)L.c_in, (int)L.c_out,
                        want_in[i], want_out[i]);
        if (!L.weight || L.bias || !L.bn_weight || !L.bn_bias || !L.bn_mean || !L.bn_var)
            return fail(DAL3_EINVAL, "pillar_pack: layer %d needs weight and BatchNorm pointers and no bias", i);
    }
    if (reinterpret_cast<uintptr_t>(out) & 15) return fail(DAL3_EINVAL, "pillar_pack: out must be 16-byte aligned");
    HIP_TRY(launch_pillar_pack(layers, n_layers, eps, out, static_cast<hipStream_t>(stream)));
    return 0;
}

static int canvas_ok(const char* who, int c_out, const float* canvas, int64_t canvas_B, int64_t ny, int64_t nx) {
    if (!canvas) return fail(DAL3_EINVAL, "%s: null canvas", who);
    if (canvas_B < 1 || ny < 1 || nx < 1 || canvas_B > DAL3_MAX_ITEMS || ny > 65536 || nx > 65536 ||
        canvas_B * c_out * ny * nx > ((int64_t)1 << 40))
        return fail(DAL3_EINVAL, "%s: bad canvas shape (canvas_B, ny, nx >= 1)", who);
    return 0;
}

extern "C" int dal3_pillar_features(const dal3_pillar_feature_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "pillar_features: null args");
    const dal3_pillar_feature_args& a = *args;
    if (a.P < 0 || a.P > DAL3_MAX_ITEMS || a.max_workgroups < 0) return fail(DAL3_EINVAL, "pillar_features: bad P / max_workgroups");
    if (a.C < 3 || a.C > 8 || a.max_points < 1 || a.max_points > 64)
        return fail(DAL3_EINVAL, "pillar_features: bad C (3 .. 8) / max_points (1 .. 64)");
    if ((a.n_layers != 1 && a.n_layers != 2) || a.c_out != 64) return fail(DAL3_EINVAL, "pillar_features: n_layers 1 or 2, c_out 64");
    if (!a.packed || (reinterpret_cast<uintptr_t>(a.packed) & 15)) return fail(DAL3_EINVAL, "pillar_features: packed is null or not 16-byte aligned");
    if (a.canvas) TRY(canvas_ok("pillar_features", a.c_out, a.canvas, a.canvas_B, a.ny, a.nx));
    else if (a.P > 0 && !a.features) return fail(DAL3_EINVAL, "pillar_features: no output (features and canvas are NULL)");
    if (a.P > 0 && (!a.voxels || !a.num_points || !a.coordinates))
        return fail(DAL3_EINVAL, "pillar_features: null voxels / num_points / coordinates");
    HIP_TRY(launch_pillar_features(args, static_cast<hipStream_t>(stream)));
    return 0;
}

static int pillar_train_ok(const char* who, const dal3_pillar_train_args& a) {
    if (a.P < 0 || a.P > DAL3_MAX_ITEMS || a.max_workgroups < 0) return fail(DAL3_EINVAL, "%s: bad P / max_workgroups", who);
    if (a.C < 3 || a.C > 8 || a.max_points < 1 || a.max_points > 64) return fail(DAL3_EINVAL, "%s: bad C (3 .. 8) / max_points (1 .. 64)", who);
    if ((a.n_layers != 1 && a.n_layers != 2) || a.c_out != 64) return fail(DAL3_EINVAL, "%s: n_layers 1 or 2, c_out 64", who);
    if (!a.layers || !(a.eps > 0.0)) return fail(DAL3_EINVAL, "%s: null layers / eps (> 0)", who);
    const int want_in[2] = {a.C + 5, 64}, want_out[2] = {a.n_layers == 1 ? 64 : 32, 64};
    for (int i = 0; i < a.n_layers; ++i) {
        const dal3_layer& L = a.layers[i];
        if (L.c_in != want_in[i] || L.c_out != want_out[i])
            return fail(DAL3_EINVAL, "%s: layer %d is %d -> %d, the kernels serve %d -> %d", who, i, (int)L.c_in, (int)L.c_out, want_in[i],
                        want_out[i]);
        if (!L.weight || L.bias || !L.bn_weight || !L.bn_bias) return fail(DAL3_EINVAL, "%s: layer %d needs weight, bn_weight, bn_bias and no bias", who, i);
    }
    if (!a.saved || (reinterpret_cast<uintptr_t>(a.saved) & 15)) return fail(DAL3_EINVAL, "%s: saved is null or not 16-byte aligned", who);
    if (a.P > 0 && (!a.voxels || !a.num_points || !a.coordinates)) return fail(DAL3_EINVAL, "%s: null voxels / num_points / coordinates", who);
    if (!a.workspace || (reinterpret_cast<uintptr_t>(a.workspace) & 7)) return fail(DAL3_EINVAL, "%s: workspace is null or not 8-byte aligned", who);
    if (a.workspace_bytes < pillar_train_workspace_bytes(a.P, a.n_layers))
        return fail(DAL3_EWORKSPACE, "%s: workspace too small (dal3_pillar_train_workspace_bytes)", who);
    return 0;
}

extern "C" size_t dal3_pillar_train_workspace_bytes(int64_t P, int n_layers) {
    if (P < 0 || P > DAL3_MAX_ITEMS || (n_layers != 1 && n_layers != 2)) return 0;
    return pillar_train_workspace_bytes(P, n_layers);
}

extern "C" int dal3_pillar_train_forward(const dal3_pillar_train_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "pillar_train_forward: null args");
    const dal3_pillar_train_args& a = *args;
    TRY(pillar_train_ok("pillar_train_forward", a));
    for (int i = 0; i < a.n_layers; ++i) {
        if (!(a.momentum[i] >= 0.0 && a.momentum[i] <= 1.0)) return fail(DAL3_EINVAL, "pillar_train_forward: momentum outside [0, 1]");
        if (!a.running_mean[i] != !a.running_var[i]) return fail(DAL3_EINVAL, "pillar_train_forward: running_mean and running_var go together");
    }
    if (a.canvas) TRY(canvas_ok("pillar_train_forward", a.c_out, a.canvas, a.canvas_B, a.ny, a.nx));
    else if (a.P > 0 && !a.features) return fail(DAL3_EINVAL, "pillar_train_forward: no output (features and canvas are NULL)");
    HIP_TRY(launch_pillar_train_forward(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_pillar_train_backward(const dal3_pillar_train_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "pillar_train_backward: null args");
    const dal3_pillar_train_args& a = *args;
    TRY(pillar_train_ok("pillar_train_backward", a));
    if (a.canvas && (a.canvas_B < 1 || a.ny < 1 || a.nx < 1)) return fail(DAL3_EINVAL, "pillar_train_backward: bad canvas shape");
    if (a.P > 0 && !a.grad) return fail(DAL3_EINVAL, "pillar_train_backward: null grad");
    for (int i = 0; i < a.n_layers; ++i)
        if (!a.dW[i] || !a.dgamma[i] || !a.dbeta[i]) return fail(DAL3_EINVAL, "pillar_train_backward: null dW / dgamma / dbeta of layer %d", i);
    HIP_TRY(launch_pillar_train_backward(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_pillar_scatter(const float* features, const int32_t* coordinates, int64_t P, const int64_t* n_pillars, int c_out,
                                   float* canvas, int64_t canvas_B, int64_t ny, int64_t nx, dal3_stream stream) {
    if (P < 0 || P > DAL3_MAX_ITEMS || c_out < 1 || c_out > 4096) return fail(DAL3_EINVAL, "pillar_scatter: bad P / c_out");
    TRY(canvas_ok("pillar_scatter", c_out, canvas, canvas_B, ny, nx));
    if (P > 0 && (!features || !coordinates)) return fail(DAL3_EINVAL, "pillar_scatter: null features / coordinates");
    HIP_TRY(launch_pillar_scatter(features, coordinates, P, n_pillars, c_out, canvas, canvas_B, ny, nx, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_voxel_mean(const float* voxels, const int32_t* num_points, int64_t P, const int64_t* n_pillars, int max_points,
                               int C, float* out, dal3_stream stream) {
    if (P < 0 || P > DAL3_MAX_ITEMS || max_points < 1 || max_points > 65536 || C < 1 || C > 64)
        return fail(DAL3_EINVAL, "voxel_mean: bad P / max_points / C");
    if (P > 0 && (!voxels || !num_points || !out)) return fail(DAL3_EINVAL, "voxel_mean: null voxels / num_points / out");
    HIP_TRY(launch_voxel_mean(voxels, num_points, P, n_pillars, max_points, C, out, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---------------------------------------------------------------------------------- the detector's dense stage
static bool conv2d_kind_ok(int kind) { return kind >= DAL3_CONV2D_3X3 && kind <= DAL3_CONV2D_DECONV4; }

// What the three pack entries of the folded MFMA layers ask of a layer (the fold: dal3_fold.h). index >= 0: the layer's
// place in a list (roi_pack's wording). The point heads' check_layer has other rules (a bias is mandatory) and is not this.
static int check_fold_layer(const char* who, const dal3_layer* L, int index, double eps, const float* out) {
    if (!L->weight) return index < 0 ? fail(DAL3_EINVAL, "%s: null weight", who) : fail(DAL3_EINVAL, "%s: layer %d has no weight", who, index);
    const bool bn = L->bn_weight || L->bn_bias || L->bn_mean || L->bn_var;
    if (bn && !(L->bn_weight && L->bn_bias && L->bn_mean && L->bn_var))
        return fail(DAL3_EINVAL, "%s: a BatchNorm needs all four of weight, bias, mean and var", who);
    if (bn && !(eps > 0.0))
        return index < 0 ? fail(DAL3_EINVAL, "%s: bad eps (> 0)", who)
                         : fail(DAL3_EINVAL, "%s: layer %d needs its BatchNorm's eps (> 0)", who, index);
    if (reinterpret_cast<uintptr_t>(out) & 15) return fail(DAL3_EINVAL, "%s: out must be 16-byte aligned", who);
    return 0;
}

extern "C" size_t dal3_conv2d_pack_floats(int kind, int c_in, int c_out) {
    if (!conv2d_kind_ok(kind) || c_in < 1 || c_in > 4096 || c_out < 1 || c_out > 4096) return 0;
    return conv2d_pack_floats(kind, c_in, c_out);
}

extern "C" int dal3_conv2d_pack(const dal3_layer* layer, int kind, double eps, float* out, dal3_stream stream) {
    if (!layer || !out) return fail(DAL3_EINVAL, "conv2d_pack: null layer / out");
    if (!conv2d_kind_ok(kind)) return fail(DAL3_EINVAL, "conv2d_pack: kind %d is no DAL3_CONV2D_* form", kind);
    if (layer->c_in < 1 || layer->c_in > 4096 || layer->c_out < 1 || layer->c_out > 4096)
        return fail(DAL3_EINVAL, "conv2d_pack: bad c_in / c_out (1 .. 4096)");
    TRY(check_fold_layer("conv2d_pack", layer, -1, eps, out));
    HIP_TRY(launch_conv2d_pack(FoldLayer(*layer, eps), kind, out, static_cast<hipStream_t>(stream)));
    return 0;
}

// what dal3_conv2d and dal3_conv2d_lp ask of the fields their args structs share
template <class Args>
static int check_conv2d_args(const char* who, const Args& a) {
    if (!conv2d_kind_ok(a.kind)) return fail(DAL3_EINVAL, "%s: kind %d is no DAL3_CONV2D_* form", who, (int)a.kind);
    const int want = a.kind == DAL3_CONV2D_DECONV2 ? 2 : a.kind == DAL3_CONV2D_DECONV4 ? 4 : 1;
    if (a.stride != want && !(a.kind == DAL3_CONV2D_3X3 && a.stride == 2))
        return fail(DAL3_EINVAL, "%s: stride %d (3x3: 1 or 2; 1x1: 1; a transposed convolution: its kernel size, 2 or 4)", who,
                    (int)a.stride);
    if ((a.relu != 0 && a.relu != 1) || a.max_workgroups < 0) return fail(DAL3_EINVAL, "%s: bad relu (0 or 1) / max_workgroups (>= 0)", who);
    if (a.c_in < 1 || a.c_in > 4096 || a.c_out < 1 || a.c_out > 4096) return fail(DAL3_EINVAL, "%s: bad c_in / c_out (1 .. 4096)", who);
    if (a.B < 0 || a.H < 0 || a.W < 0 || a.B > 65535 || a.H > 65535 || a.W > 65535)
        return fail(DAL3_EINVAL, "%s: bad B / H / W (0 .. 65535)", who);
    if (a.y_channel_offset < 0 || a.y_channels < 1 || (int64_t)a.y_channel_offset + a.c_out > a.y_channels)
        return fail(DAL3_EINVAL, "%s: channels %d .. %lld lie outside the output's %d", who, (int)a.y_channel_offset,
                    (long long)a.y_channel_offset + a.c_out, (int)a.y_channels);
    if (!a.x.data || !a.y.data) return fail(DAL3_EINVAL, "%s: null x / y", who);
    if (!a.packed || (reinterpret_cast<uintptr_t>(a.packed) & 15)) return fail(DAL3_EINVAL, "%s: packed is null or not 16-byte aligned", who);
    return 0;
}

extern "C" int dal3_conv2d(const dal3_conv2d_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "conv2d: null args");
    TRY(check_conv2d_args("conv2d", *args));
    HIP_TRY(launch_conv2d(args, static_cast<hipStream_t>(stream)));
    return 0;
}

// ... and on 16-bit MFMA operands (dal3_conv2d_lp.hip)
static bool conv2d_lp_dtype_ok(int dtype) { return dtype == DAL3_F16 || dtype == DAL3_BF16; }

extern "C" size_t dal3_conv2d_lp_pack_bytes(int kind, int c_in, int c_out) {
    if (!conv2d_kind_ok(kind) || c_in < 1 || c_in > 4096 || c_out < 1 || c_out > 4096) return 0;
    return conv2d_lp_pack_bytes(kind, c_in, c_out);
}

extern "C" int dal3_conv2d_lp_pack(const dal3_layer* layer, int kind, double eps, int dtype, void* out, dal3_stream stream) {
    if (!layer || !out) return fail(DAL3_EINVAL, "conv2d_lp_pack: null layer / out");
    if (!conv2d_kind_ok(kind)) return fail(DAL3_EINVAL, "conv2d_lp_pack: kind %d is no DAL3_CONV2D_* form", kind);
    if (!conv2d_lp_dtype_ok(dtype)) return fail(DAL3_EINVAL, "conv2d_lp_pack: dtype %d (DAL3_F16 or DAL3_BF16)", dtype);
    if (layer->c_in < 1 || layer->c_in > 4096 || layer->c_out < 1 || layer->c_out > 4096)
        return fail(DAL3_EINVAL, "conv2d_lp_pack: bad c_in / c_out (1 .. 4096)");
    TRY(check_fold_layer("conv2d_lp_pack", layer, -1, eps, static_cast<const float*>(out)));
    HIP_TRY(launch_conv2d_lp_pack(FoldLayer(*layer, eps), kind, dtype, out, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_conv2d_lp(const dal3_conv2d_lp_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "conv2d_lp: null args");
    if (!conv2d_lp_dtype_ok(args->dtype)) return fail(DAL3_EINVAL, "conv2d_lp: dtype %d (DAL3_F16 or DAL3_BF16)", (int)args->dtype);
    if (args->reserved != 0) return fail(DAL3_EINVAL, "conv2d_lp: reserved must be 0");
    TRY(check_conv2d_args("conv2d_lp", *args));
    HIP_TRY(launch_conv2d_lp(args, static_cast<hipStream_t>(stream)));
    return 0;
}

// ... and their backward pass (dal3_conv2d_train.hip)
static bool conv2d_dgrad_kind_ok(int kind) { return kind == DAL3_CONV2D_3X3 || kind == DAL3_CONV2D_DECONV2 || kind == DAL3_CONV2D_DECONV4; }
static bool conv2d_width_ok(int c) { return c >= 1 && c <= 4096; }
static bool conv2d_extent_ok(int64_t v) { return v >= 0 && v <= 65535; }

extern "C" size_t dal3_conv2d_dgrad_pack_floats(int kind, int c_in, int c_out) {
    if (!conv2d_dgrad_kind_ok(kind) || !conv2d_width_ok(c_in) || !conv2d_width_ok(c_out)) return 0;
    return conv2d_dgrad_pack_floats(kind, c_in, c_out);
}

extern "C" int dal3_conv2d_dgrad_pack(const float* weight, int kind, int c_in, int c_out, float* out, dal3_stream stream) {
    if (!weight || !out) return fail(DAL3_EINVAL, "conv2d_dgrad_pack: null weight / out");
    if (!conv2d_dgrad_kind_ok(kind))
        return fail(DAL3_EINVAL, "conv2d_dgrad_pack: kind %d (DAL3_CONV2D_3X3 of stride 2, _DECONV2 or _DECONV4: the other forms' data "
                    "gradient is dal3_conv2d on the transposed pack)", kind);
    if (!conv2d_width_ok(c_in) || !conv2d_width_ok(c_out)) return fail(DAL3_EINVAL, "conv2d_dgrad_pack: bad c_in / c_out (1 .. 4096)");
    if (reinterpret_cast<uintptr_t>(out) & 15) return fail(DAL3_EINVAL, "conv2d_dgrad_pack: out must be 16-byte aligned");
    HIP_TRY(launch_conv2d_dgrad_pack(weight, kind, c_in, c_out, out, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_conv2d_dgrad(const dal3_conv2d_dgrad_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "conv2d_dgrad: null args");
    const dal3_conv2d_dgrad_args& a = *args;
    if (!conv2d_dgrad_kind_ok(a.kind))
        return fail(DAL3_EINVAL, "conv2d_dgrad: kind %d (DAL3_CONV2D_3X3 of stride 2, _DECONV2 or _DECONV4: the other forms' data gradient "
                    "is dal3_conv2d on the transposed pack)", (int)a.kind);
    if (a.stride != (a.kind == DAL3_CONV2D_DECONV4 ? 4 : 2))
        return fail(DAL3_EINVAL, "conv2d_dgrad: stride %d (3x3: 2; a transposed convolution: its kernel size, 2 or 4)", (int)a.stride);
    if (a.max_workgroups < 0 || a.reserved) return fail(DAL3_EINVAL, "conv2d_dgrad: bad max_workgroups (>= 0) / reserved");
    if (!conv2d_width_ok(a.c_in) || !conv2d_width_ok(a.c_out)) return fail(DAL3_EINVAL, "conv2d_dgrad: bad c_in / c_out (1 .. 4096)");
    if (!conv2d_extent_ok(a.B) || !conv2d_extent_ok(a.H) || !conv2d_extent_ok(a.W)) return fail(DAL3_EINVAL, "conv2d_dgrad: bad B / H / W (0 .. 65535)");
    if (a.kind != DAL3_CONV2D_3X3 && (a.H * a.stride > 65535 || a.W * a.stride > 65535))
        return fail(DAL3_EINVAL, "conv2d_dgrad: dy's extent exceeds 65535");
    if (!a.dy.data || !a.dx.data) return fail(DAL3_EINVAL, "conv2d_dgrad: null dy / dx");
    if (!a.packed || (reinterpret_cast<uintptr_t>(a.packed) & 15)) return fail(DAL3_EINVAL, "conv2d_dgrad: packed is null or not 16-byte aligned");
    HIP_TRY(launch_conv2d_dgrad(args, static_cast<hipStream_t>(stream)));
    return 0;
}

static bool conv2d_wgrad_form_ok(int kind, int stride) {
    if (!conv2d_kind_ok(kind)) return false;
    const int want = kind == DAL3_CONV2D_DECONV2 ? 2 : kind == DAL3_CONV2D_DECONV4 ? 4 : 1;
    return stride == want || (kind == DAL3_CONV2D_3X3 && stride == 2);
}

extern "C" size_t dal3_conv2d_wgrad_workspace_bytes(int kind, int stride, int c_in, int c_out, int64_t B, int64_t H, int64_t W) {
    if (!conv2d_wgrad_form_ok(kind, stride) || !conv2d_width_ok(c_in) || !conv2d_width_ok(c_out) || !conv2d_extent_ok(B) ||
        !conv2d_extent_ok(H) || !conv2d_extent_ok(W))
        return 0;
    return conv2d_wgrad_workspace_bytes(kind, stride, c_in, c_out, B, H, W);
}

extern "C" int dal3_conv2d_wgrad(const dal3_conv2d_wgrad_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "conv2d_wgrad: null args");
    const dal3_conv2d_wgrad_args& a = *args;
    if (!conv2d_wgrad_form_ok(a.kind, a.stride))
        return fail(DAL3_EINVAL, "conv2d_wgrad: kind %d with stride %d (3x3: 1 or 2; 1x1: 1; a transposed convolution: its kernel size, 2 or 4)",
                    (int)a.kind, (int)a.stride);
    if (a.max_workgroups < 0 || a.reserved) return fail(DAL3_EINVAL, "conv2d_wgrad: bad max_workgroups (>= 0) / reserved");
    if (!conv2d_width_ok(a.c_in) || !conv2d_width_ok(a.c_out)) return fail(DAL3_EINVAL, "conv2d_wgrad: bad c_in / c_out (1 .. 4096)");
    if (!conv2d_extent_ok(a.B) || !conv2d_extent_ok(a.H) || !conv2d_extent_ok(a.W)) return fail(DAL3_EINVAL, "conv2d_wgrad: bad B / H / W (0 .. 65535)");
    if (a.kind >= DAL3_CONV2D_DECONV2 && (a.H * a.stride > 65535 || a.W * a.stride > 65535))
        return fail(DAL3_EINVAL, "conv2d_wgrad: dy's extent exceeds 65535");
    if (!a.dw) return fail(DAL3_EINVAL, "conv2d_wgrad: null dw");
    if (a.B > 0 && a.H > 0 && a.W > 0) {
        if (!a.x.data || !a.dy.data) return fail(DAL3_EINVAL, "conv2d_wgrad: null x / dy");
        if (!a.workspace) return fail(DAL3_EINVAL, "conv2d_wgrad: null workspace");
        if (a.workspace_bytes < conv2d_wgrad_workspace_bytes(a.kind, a.stride, a.c_in, a.c_out, a.B, a.H, a.W))
            return fail(DAL3_EWORKSPACE, "conv2d_wgrad: workspace too small (dal3_conv2d_wgrad_workspace_bytes)");
        if (reinterpret_cast<uintptr_t>(a.workspace) & 7) return fail(DAL3_EINVAL, "conv2d_wgrad: workspace must be 8-byte aligned");
    }
    HIP_TRY(launch_conv2d_wgrad(args, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---------------------------------------------------------------------------------- the sparse 3-D middle
static int sp_grid_ok(const char* who, int64_t B, const int32_t* shape) {
    if (B < 1 || B > 65535) return fail(DAL3_EINVAL, "%s: bad B (1 .. 65535)", who);
    for (int j = 0; j < 3; ++j)
        if (shape[j] < 1 || shape[j] > 65536) return fail(DAL3_EINVAL, "%s: every axis of a grid needs 1 .. 65536 cells", who);
    const int64_t cells = (int64_t)shape[0] * shape[1] * shape[2];
    if (cells >= 2147483647 || cells >= 2147483647 / B)
        return fail(DAL3_EINVAL, "%s: the (sample, cell) key needs B * D * H * W < 2^31 - 1 (split the batch)", who);
    return 0;
}

static int sp_window_ok(const char* who, const int32_t* in, const int32_t* out, const int32_t* k, const int32_t* s, const int32_t* p) {
    for (int j = 0; j < 3; ++j) {
        if (k[j] < 1 || k[j] > 3 || s[j] < 1 || s[j] > 3 || p[j] < 0 || p[j] > 2)
            return fail(DAL3_EINVAL, "%s: kernel 1 .. 3, stride 1 .. 3, padding 0 .. 2 per axis", who);
        if (in[j] + 2 * p[j] < k[j] || out[j] != (in[j] + 2 * p[j] - k[j]) / s[j] + 1)
            return fail(DAL3_EINVAL, "%s: out_shape[%d] must be floor((in + 2 padding - kernel) / stride) + 1", who, j);
    }
    return 0;
}

static bool sp_cap_ok(int64_t c) { return c >= 0 && c <= ((int64_t)1 << 28); }

extern "C" size_t dal3_sp_sort_workspace_bytes(int64_t capacity) { return sp_cap_ok(capacity) ? sp_sort_workspace_bytes(capacity) : 0; }

extern "C" int dal3_sp_sort(const dal3_sp_sort_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "sp_sort: null args");
    const dal3_sp_sort_args& a = *args;
    TRY(sp_grid_ok("sp_sort", a.B, a.shape));
    if (!sp_cap_ok(a.capacity) || a.max_workgroups < 0 || a.reserved) return fail(DAL3_EINVAL, "sp_sort: bad capacity / max_workgroups / reserved");
    if (!a.status) return fail(DAL3_EINVAL, "sp_sort: null status");
    if (a.capacity > 0) {
        if (!a.indices || !a.sorted_key || !a.sorted_pos || !a.workspace) return fail(DAL3_EINVAL, "sp_sort: null indices / sorted_key / sorted_pos / workspace");
        if (a.workspace_bytes < sp_sort_workspace_bytes(a.capacity)) return fail(DAL3_EWORKSPACE, "sp_sort: workspace too small (dal3_sp_sort_workspace_bytes)");
        if (reinterpret_cast<uintptr_t>(a.workspace) & 7) return fail(DAL3_EINVAL, "sp_sort: workspace must be 8-byte aligned");
    }
    HIP_TRY(launch_sp_sort(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_sp_downsample_workspace_bytes(int64_t in_capacity, int candidates) {
    if (!sp_cap_ok(in_capacity) || candidates < 1 || candidates > 27 || !sp_cap_ok(in_capacity * candidates)) return 0;
    return sp_downsample_workspace_bytes(in_capacity, candidates);
}

extern "C" int dal3_sp_downsample(const dal3_sp_downsample_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "sp_downsample: null args");
    const dal3_sp_downsample_args& a = *args;
    TRY(sp_grid_ok("sp_downsample", a.B, a.in_shape));
    TRY(sp_window_ok("sp_downsample", a.in_shape, a.out_shape, a.kernel, a.stride, a.padding));
    TRY(sp_grid_ok("sp_downsample", a.B, a.out_shape));
    const int cand = sp_candidates(a.kernel, a.stride);
    if (!sp_cap_ok(a.in_capacity) || !sp_cap_ok(a.out_capacity) || !sp_cap_ok(a.in_capacity * cand) || a.max_workgroups < 0 || a.reserved)
        return fail(DAL3_EINVAL, "sp_downsample: bad capacity / max_workgroups / reserved");
    if (!a.status || !a.n_out) return fail(DAL3_EINVAL, "sp_downsample: null status / n_out");
    if (a.out_capacity > 0 && (!a.out_indices || !a.out_key)) return fail(DAL3_EINVAL, "sp_downsample: null out_indices / out_key");
    if (a.in_capacity > 0) {
        if (!a.in_indices || !a.workspace) return fail(DAL3_EINVAL, "sp_downsample: null in_indices / workspace");
        if (a.workspace_bytes < sp_downsample_workspace_bytes(a.in_capacity, cand))
            return fail(DAL3_EWORKSPACE, "sp_downsample: workspace too small (dal3_sp_downsample_workspace_bytes)");
        if (reinterpret_cast<uintptr_t>(a.workspace) & 7) return fail(DAL3_EINVAL, "sp_downsample: workspace must be 8-byte aligned");
    }
    HIP_TRY(launch_sp_downsample(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_sp_table(const dal3_sp_table_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "sp_table: null args");
    const dal3_sp_table_args& a = *args;
    TRY(sp_grid_ok("sp_table", a.B, a.in_shape));
    TRY(sp_window_ok("sp_table", a.in_shape, a.out_shape, a.kernel, a.stride, a.padding));
    TRY(sp_grid_ok("sp_table", a.B, a.out_shape));
    if (!sp_cap_ok(a.in_capacity) || !sp_cap_ok(a.out_capacity) || !sp_cap_ok(a.out_capacity * 27) || a.max_workgroups < 0 || a.reserved)
        return fail(DAL3_EINVAL, "sp_table: bad capacity / max_workgroups / reserved");
    if (a.out_capacity > 0 && (!a.out_indices || !a.table)) return fail(DAL3_EINVAL, "sp_table: null out_indices / table");
    if (a.out_capacity > 0 && a.in_capacity > 0 && !a.in_key) return fail(DAL3_EINVAL, "sp_table: null in_key");
    HIP_TRY(launch_sp_table(args, static_cast<hipStream_t>(stream)));
    return 0;
}

static bool sp_channels_ok(int c_in, int c_out) {
    const bool in = (c_in >= 1 && c_in <= 8) || c_in == 16 || c_in == 32 || c_in == 64 || c_in == 128;
    return in && (c_out == 16 || c_out == 32 || c_out == 64 || c_out == 128);
}

extern "C" size_t dal3_sp_conv_pack_floats(int taps, int c_in, int c_out) {
    if (taps < 1 || taps > 27 || !sp_channels_ok(c_in, c_out)) return 0;
    return sp_conv_pack_floats(taps, c_in, c_out);
}

extern "C" int dal3_sp_conv_pack(const dal3_layer* layer, int taps, double eps, float* out, int32_t* status, dal3_stream stream) {
    if (!layer || !out) return fail(DAL3_EINVAL, "sp_conv_pack: null layer / out");
    if (taps < 1 || taps > 27) return fail(DAL3_EINVAL, "sp_conv_pack: %d taps (1 .. 27)", taps);
    if (!sp_channels_ok(layer->c_in, layer->c_out))
        return fail(DAL3_EINVAL, "sp_conv_pack: %d -> %d channels (c_in 1 .. 8, 16, 32, 64, 128; c_out 16, 32, 64, 128)", (int)layer->c_in,
                    (int)layer->c_out);
    TRY(check_fold_layer("sp_conv_pack", layer, -1, eps, out));
    HIP_TRY(launch_sp_conv_pack(FoldLayer(*layer, eps), taps, out, status, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_sp_conv(const dal3_sp_conv_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "sp_conv: null args");
    const dal3_sp_conv_args& a = *args;
    if (a.taps < 1 || a.taps > 27 || !sp_channels_ok(a.c_in, a.c_out))
        return fail(DAL3_EINVAL, "sp_conv: %d taps, %d -> %d channels (taps 1 .. 27; c_in 1 .. 8, 16, 32, 64, 128; c_out 16, 32, 64, 128)", (int)a.taps,
                    (int)a.c_in, (int)a.c_out);
    if ((a.relu != 0 && a.relu != 1) || a.center_tap < -1 || a.center_tap >= a.taps || a.max_workgroups < 0 || a.reserved || a.reserved2)
        return fail(DAL3_EINVAL, "sp_conv: bad relu (0 or 1) / center_tap (-1 .. taps - 1) / max_workgroups (>= 0) / reserved");
    if (!sp_cap_ok(a.in_capacity) || !sp_cap_ok(a.out_capacity) || !sp_cap_ok(a.out_capacity * 27)) return fail(DAL3_EINVAL, "sp_conv: bad capacity");
    if (!a.status) return fail(DAL3_EINVAL, "sp_conv: null status");
    if (!a.packed || (reinterpret_cast<uintptr_t>(a.packed) & 15)) return fail(DAL3_EINVAL, "sp_conv: packed is null or not 16-byte aligned");
    if (a.canvas) {
        if (!a.out_indices && a.out_capacity > 0) return fail(DAL3_EINVAL, "sp_conv: a canvas needs out_indices");
        if (a.canvas_B < 1 || a.canvas_B > 65535 || a.canvas_shape[0] < 1 || a.canvas_shape[1] < 1 || a.canvas_shape[2] < 1 ||
            a.canvas_shape[0] > 65536 || a.canvas_shape[1] > 65536 || a.canvas_shape[2] > 65536 ||
            a.canvas_B * a.c_out * a.canvas_shape[0] * a.canvas_shape[1] * a.canvas_shape[2] > ((int64_t)1 << 40))
            return fail(DAL3_EINVAL, "sp_conv: bad canvas shape (canvas_B, D, H, W >= 1)");
    } else if (a.out_capacity > 0 && !a.y) {
        return fail(DAL3_EINVAL, "sp_conv: no output (y and canvas are NULL)");
    }
    if (a.out_capacity > 0) {
        if (!a.table || (a.in_capacity > 0 && !a.x)) return fail(DAL3_EINVAL, "sp_conv: null table / x");
        if (((a.c_in > 8 ? reinterpret_cast<uintptr_t>(a.x) : 0) | reinterpret_cast<uintptr_t>(a.y) | reinterpret_cast<uintptr_t>(a.residual)) & 15)
            return fail(DAL3_EINVAL, "sp_conv: x (with 16 or more channels), y and residual must be 16-byte aligned");
    }
    HIP_TRY(launch_sp_conv(args, static_cast<hipStream_t>(stream)));
    return 0;
}

// ... and on 16-bit MFMA operands (dal3_spconv_lp.hip)
extern "C" size_t dal3_sp_conv_lp_pack_bytes(int taps, int c_in, int c_out) {
    if (taps < 1 || taps > 27 || !sp_channels_ok(c_in, c_out)) return 0;
    return sp_conv_lp_pack_bytes(taps, c_in, c_out);
}

extern "C" int dal3_sp_conv_lp_pack(const dal3_layer* layer, int taps, double eps, int dtype, void* out, int32_t* status,
                                    dal3_stream stream) {
    if (!layer || !out) return fail(DAL3_EINVAL, "sp_conv_lp_pack: null layer / out");
    if (!conv2d_lp_dtype_ok(dtype)) return fail(DAL3_EINVAL, "sp_conv_lp_pack: dtype %d (DAL3_F16 or DAL3_BF16)", dtype);
    if (taps < 1 || taps > 27) return fail(DAL3_EINVAL, "sp_conv_lp_pack: %d taps (1 .. 27)", taps);
    if (!sp_channels_ok(layer->c_in, layer->c_out))
        return fail(DAL3_EINVAL, "sp_conv_lp_pack: %d -> %d channels (c_in 1 .. 8, 16, 32, 64, 128; c_out 16, 32, 64, 128)",
                    (int)layer->c_in, (int)layer->c_out);
    TRY(check_fold_layer("sp_conv_lp_pack", layer, -1, eps, static_cast<const float*>(out)));
    HIP_TRY(launch_sp_conv_lp_pack(FoldLayer(*layer, eps), taps, dtype, out, status, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_sp_conv_lp(const dal3_sp_conv_lp_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "sp_conv_lp: null args");
    const dal3_sp_conv_lp_args& a = *args;
    if (!conv2d_lp_dtype_ok(a.dtype)) return fail(DAL3_EINVAL, "sp_conv_lp: dtype %d (DAL3_F16 or DAL3_BF16)", (int)a.dtype);
    if (a.taps < 1 || a.taps > 27 || !sp_channels_ok(a.c_in, a.c_out))
        return fail(DAL3_EINVAL, "sp_conv_lp: %d taps, %d -> %d channels (taps 1 .. 27; c_in 1 .. 8, 16, 32, 64, 128; c_out 16, 32, 64, 128)",
                    (int)a.taps, (int)a.c_in, (int)a.c_out);
    if ((a.relu != 0 && a.relu != 1) || a.center_tap < -1 || a.center_tap >= a.taps || a.max_workgroups < 0 || a.reserved || a.reserved2)
        return fail(DAL3_EINVAL, "sp_conv_lp: bad relu (0 or 1) / center_tap (-1 .. taps - 1) / max_workgroups (>= 0) / reserved");
    if (!sp_cap_ok(a.in_capacity) || !sp_cap_ok(a.out_capacity) || !sp_cap_ok(a.out_capacity * 27)) return fail(DAL3_EINVAL, "sp_conv_lp: bad capacity");
    if (!a.status) return fail(DAL3_EINVAL, "sp_conv_lp: null status");
    if (!a.packed || (reinterpret_cast<uintptr_t>(a.packed) & 15)) return fail(DAL3_EINVAL, "sp_conv_lp: packed is null or not 16-byte aligned");
    if (a.x && a.x16) return fail(DAL3_EINVAL, "sp_conv_lp: both x and x16 are given (exactly one)");
    if (a.x16 && a.c_in <= 8) return fail(DAL3_EINVAL, "sp_conv_lp: x16 needs c_in 16, 32, 64 or 128 (c_in %d comes as float32 x)", (int)a.c_in);
    if (a.canvas) {
        if (!a.out_indices && a.out_capacity > 0) return fail(DAL3_EINVAL, "sp_conv_lp: a canvas needs out_indices");
        if (a.canvas_B < 1 || a.canvas_B > 65535 || a.canvas_shape[0] < 1 || a.canvas_shape[1] < 1 || a.canvas_shape[2] < 1 ||
            a.canvas_shape[0] > 65536 || a.canvas_shape[1] > 65536 || a.canvas_shape[2] > 65536 ||
            a.canvas_B * a.c_out * a.canvas_shape[0] * a.canvas_shape[1] * a.canvas_shape[2] > ((int64_t)1 << 40))
            return fail(DAL3_EINVAL, "sp_conv_lp: bad canvas shape (canvas_B, D, H, W >= 1)");
    } else if (a.out_capacity > 0 && !a.y && !a.y16) {
        return fail(DAL3_EINVAL, "sp_conv_lp: no output (y, y16 and canvas are NULL)");
    }
    if (a.out_capacity > 0) {
        if (!a.table) return fail(DAL3_EINVAL, "sp_conv_lp: null table");
        if (a.in_capacity > 0 && !a.x && !a.x16) return fail(DAL3_EINVAL, "sp_conv_lp: neither x nor x16 is given (exactly one)");
        if (((a.c_in > 8 ? reinterpret_cast<uintptr_t>(a.x) : 0) | reinterpret_cast<uintptr_t>(a.x16) | reinterpret_cast<uintptr_t>(a.y) |
             reinterpret_cast<uintptr_t>(a.y16) | reinterpret_cast<uintptr_t>(a.residual)) & 15)
            return fail(DAL3_EINVAL, "sp_conv_lp: x (with 16 or more channels), x16, y, y16 and residual must be 16-byte aligned");
    }
    HIP_TRY(launch_sp_conv_lp(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_sp_table_transposed(const dal3_sp_table_transposed_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "sp_table_transposed: null args");
    const dal3_sp_table_transposed_args& a = *args;
    TRY(sp_grid_ok("sp_table_transposed", a.B, a.in_shape));
    TRY(sp_window_ok("sp_table_transposed", a.in_shape, a.out_shape, a.kernel, a.stride, a.padding));
    TRY(sp_grid_ok("sp_table_transposed", a.B, a.out_shape));
    if (!sp_cap_ok(a.in_capacity) || !sp_cap_ok(a.out_capacity) || !sp_cap_ok(a.in_capacity * 27) || a.max_workgroups < 0 || a.reserved)
        return fail(DAL3_EINVAL, "sp_table_transposed: bad capacity / max_workgroups / reserved");
    if (a.in_capacity > 0 && (!a.in_indices || !a.table)) return fail(DAL3_EINVAL, "sp_table_transposed: null in_indices / table");
    if (a.in_capacity > 0 && a.out_capacity > 0 && !a.out_key) return fail(DAL3_EINVAL, "sp_table_transposed: null out_key");
    HIP_TRY(launch_sp_table_transposed(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_sp_wgrad_workspace_bytes(int taps, int c_in, int c_out, int64_t out_capacity) {
    if (taps < 1 || taps > 27 || !sp_channels_ok(c_in, c_out) || !sp_cap_ok(out_capacity)) return 0;
    return sp_wgrad_workspace_bytes(taps, c_in, c_out, out_capacity);
}

extern "C" int dal3_sp_wgrad(const dal3_sp_wgrad_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "sp_wgrad: null args");
    const dal3_sp_wgrad_args& a = *args;
    if (a.taps < 1 || a.taps > 27 || !sp_channels_ok(a.c_in, a.c_out))
        return fail(DAL3_EINVAL, "sp_wgrad: %d taps, %d -> %d channels (taps 1 .. 27; c_in 1 .. 8, 16, 32, 64, 128; c_out 16, 32, 64, 128)",
                    (int)a.taps, (int)a.c_in, (int)a.c_out);
    if (a.max_workgroups < 0 || a.reserved) return fail(DAL3_EINVAL, "sp_wgrad: bad max_workgroups (>= 0) / reserved");
    if (!sp_cap_ok(a.in_capacity) || !sp_cap_ok(a.out_capacity) || !sp_cap_ok(a.out_capacity * 27)) return fail(DAL3_EINVAL, "sp_wgrad: bad capacity");
    if (!a.dw) return fail(DAL3_EINVAL, "sp_wgrad: null dw");
    if (a.out_capacity > 0) {
        if (!a.table || !a.dy || (a.in_capacity > 0 && !a.x)) return fail(DAL3_EINVAL, "sp_wgrad: null table / dy / x");
        if (!a.workspace) return fail(DAL3_EINVAL, "sp_wgrad: null workspace");
        if (a.workspace_bytes < sp_wgrad_workspace_bytes(a.taps, a.c_in, a.c_out, a.out_capacity))
            return fail(DAL3_EWORKSPACE, "sp_wgrad: workspace too small (dal3_sp_wgrad_workspace_bytes)");
        if (reinterpret_cast<uintptr_t>(a.workspace) & 7) return fail(DAL3_EINVAL, "sp_wgrad: workspace must be 8-byte aligned");
    }
    HIP_TRY(launch_sp_wgrad(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_crop_workspace_bytes(int64_t K_total, int64_t max_points_per_frame) {
    if (K_total <= 0 || max_points_per_frame < 0) return 0;
    return crop_workspace_bytes(K_total, max_points_per_frame);
}

static int crop_args_ok(const float* points, const int64_t* point_offsets, const double* planes, const float* spheres,
                        const int64_t* box_offsets, int F, int64_t K_total, int64_t max_pts, const void* ws,
                        size_t ws_bytes) {
    if (!point_offsets || !box_offsets || F <= 0 || F > 65535 || K_total < 0 || max_pts < 0)
        return fail(DAL3_EINVAL, "crop: bad argument (1 <= F <= 65535)");
    if (K_total > 0 && max_pts > 0 && (!points || !planes || !spheres))
        return fail(DAL3_EINVAL, "crop: null points / planes / spheres");
    if (K_total > 0 && (!ws || ws_bytes < crop_workspace_bytes(K_total, max_pts)))
        return fail(DAL3_EWORKSPACE, "crop: workspace smaller than dal3_crop_workspace_bytes()");
    return 0;
}

extern "C" int dal3_crop_count(const float* points, const int64_t* point_offsets, const double* planes,
                               const float* spheres, const int64_t* box_offsets, int F, int64_t K_total,
                               int64_t max_points_per_frame, int64_t* counts, void* workspace, size_t workspace_bytes,
                               dal3_stream stream) {
    if (int e = crop_args_ok(points, point_offsets, planes, spheres, box_offsets, F, K_total, max_points_per_frame,
                             workspace, workspace_bytes))
        return e;
    if (K_total > 0 && !counts) return fail(DAL3_EINVAL, "crop_count: null counts");
    HIP_TRY(launch_crop_count(points, point_offsets, planes, spheres, box_offsets, F, K_total, max_points_per_frame, counts,
                              static_cast<int32_t*>(workspace), static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_crop_fill(const float* points, const int64_t* point_offsets, const double* planes,
                              const float* spheres, const int64_t* box_offsets, int F, int64_t K_total,
                              int64_t max_points_per_frame, const double* pose, const int64_t* counts,
                              const int64_t* box_start, double* out_points, int32_t* out_index, int64_t out_capacity,
                              const void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (int e = crop_args_ok(points, point_offsets, planes, spheres, box_offsets, F, K_total, max_points_per_frame,
                             workspace, workspace_bytes))
        return e;
    if (K_total > 0 && (!pose || !counts || !box_start || !out_points || out_capacity < 0))
        return fail(DAL3_EINVAL, "crop_fill: null pose / counts / box_start / out, or a negative out_capacity");
    HIP_TRY(launch_crop_fill(points, point_offsets, planes, spheres, box_offsets, F, K_total, max_points_per_frame, pose,
                             counts, box_start, static_cast<const int32_t*>(workspace), out_points, out_index, out_capacity,
                             static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_crop_starts(const int64_t* counts, const int64_t* order, int64_t K_total, int64_t* box_start,
                                int64_t* out_offsets, dal3_stream stream) {
    if (K_total < 0 || !box_start || (K_total > 0 && !counts))
        return fail(DAL3_EINVAL, "crop_starts: null counts / box_start or K_total < 0");
    HIP_TRY(launch_crop_starts(counts, order, K_total, box_start, out_offsets, -1, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_crop_starts_capped(const int64_t* counts, const int64_t* order, int64_t K_total, int64_t* box_start,
                                       int64_t* out_offsets, int64_t out_capacity, dal3_stream stream) {
    if (K_total < 0 || !box_start || (K_total > 0 && !counts) || out_capacity < 0)
        return fail(DAL3_EINVAL, "crop_starts_capped: null counts / box_start, K_total < 0 or out_capacity < 0");
    HIP_TRY(launch_crop_starts(counts, order, K_total, box_start, out_offsets, out_capacity, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_writeback_boxes(const double* final_boxes, const int32_t* final_idx, const double* pose_best,
                                    const double* pose_inv, const double* track_box, float* det,
                                    const int64_t* det_start, const int32_t* det_count, const uint8_t* active, int P,
                                    int64_t n_det, int32_t* match, int32_t* owner, dal3_stream stream) {
    if (!final_boxes || !final_idx || !pose_inv || !track_box || !det || !det_start || !det_count || !active || !match ||
        !owner || P <= 0 || n_det <= 0)
        return fail(DAL3_EINVAL, "writeback_boxes: bad argument");
    HIP_TRY(launch_writeback(final_boxes, final_idx, pose_best, pose_inv, track_box, det, det_start, det_count, active, P,
                             n_det, match, owner, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---------------------------------------------------------------------------------------------- training blocks (N4)
static bool mult32(int64_t v) { return v > 0 && v % 32 == 0; }

extern "C" int dal3_tr_linear(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                              int relu_in, const float* W, int64_t ldw, int transpose_w, const float* bias, int64_t seg,
                              int c_out, float* z, int64_t ldz, int accumulate, void* workspace, size_t workspace_bytes,
                              dal3_stream stream) {
    if (!a || !W || !z || !mult32(M) || !mult32(c_in) || !mult32(c_out) || lda < c_in || ldz < c_out || lda % 4 || ldz % 4 ||
        (!transpose_w && (ldw < c_in || ldw % 4)) || (transpose_w && ldw < c_out) || (scale && !shift) || seg < 0)
        return fail(DAL3_EINVAL, "tr_linear: bad argument (M, c_in, c_out multiples of 32; strides multiples of 4)");
    const size_t need = tr_linear_workspace_bytes(c_in, c_out);
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return fail(DAL3_EWORKSPACE, "tr_linear: workspace smaller than dal3_tr_linear_workspace_bytes() or not 16-byte aligned");
    HIP_TRY(launch_tr_linear(a, M, c_in, lda, scale, shift, relu_in, W, ldw, transpose_w, bias, seg, c_out, z, ldz,
                             accumulate, need ? static_cast<float*>(workspace) : nullptr, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_linear_pack_layout(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, int has_act) {
    if (!mult32(M) || !mult32(c_in) || !mult32(c_out)) return 0;
    return tr_linear_pack_mtb(M, c_in, seg, c_out, accumulate, has_act);
}

extern "C" int dal3_tr_pack_many(const dal3_tr_pack_item* items, int n, dal3_stream stream) {
    if (!items || n <= 0 || n > 48) return fail(DAL3_EINVAL, "tr_pack_many: 1 .. 48 items");
    for (int i = 0; i < n; ++i) {
        const dal3_tr_pack_item& t = items[i];
        const int mtb = t.mtb & 0xff;
        if ((t.mtb & ~0x1ff) || ((t.mtb & 0x100) && mtb != 8)) return fail(DAL3_EINVAL, "tr_pack_many: bad layout code in item %d", i);
        if (!t.W || !t.out || !mult32(t.c_in) || !mult32(t.c_out) || mtb <= 0 || (t.c_out / 32) % mtb != 0 ||
            (reinterpret_cast<uintptr_t>(t.out) & 15) || (!t.transpose_w && t.ldw < t.c_in) || (t.transpose_w && t.ldw < t.c_out))
            return fail(DAL3_EINVAL, "tr_pack_many: bad item %d", i);
    }
    HIP_TRY(launch_tr_pack_many(items, n, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_linear_prepacked(const float* a, int64_t M, int c_in, int64_t lda, const float* scale,
                                        const float* shift, int relu_in, const float* W, int64_t ldw, int transpose_w,
                                        const float* bias, int64_t seg, int c_out, float* z, int64_t ldz, int accumulate,
                                        const void* packed, dal3_stream stream) {
    if (!a || !W || !z || !mult32(M) || !mult32(c_in) || !mult32(c_out) || lda < c_in || ldz < c_out || lda % 4 || ldz % 4 ||
        (scale && !shift) || seg < 0 || !packed || (reinterpret_cast<uintptr_t>(packed) & 15))
        return fail(DAL3_EINVAL, "tr_linear_prepacked: bad argument");
    if (tr_linear_pack_mtb(M, c_in, seg, c_out, accumulate, scale != nullptr) == 0)
        return fail(DAL3_EINVAL, "tr_linear_prepacked: this call reads no packed image (dal3_tr_linear_pack_layout() == 0)");
    HIP_TRY(launch_tr_linear(a, M, c_in, lda, scale, shift, relu_in, W, ldw, transpose_w, bias, seg, c_out, z, ldz, accumulate,
                             const_cast<float*>(static_cast<const float*>(packed)), static_cast<hipStream_t>(stream), true));
    return 0;
}

extern "C" size_t dal3_tr_linear_red_workspace_bytes(int64_t rows, int c_out) {
    if (rows <= 0 || c_out <= 0) return 0;
    const size_t a = tr_colred_workspace_bytes(rows, c_out), b = tr_linear_red_workspace_bytes();
    return a > b ? a : b;
}

static int tr_linear_red_args_ok(const float* a, int64_t M, int c_in, int64_t lda, int c_out, const float* z, int64_t ldz,
                                 const void* packed, int64_t rows) {
    return a && z && mult32(M) && mult32(c_in) && mult32(c_out) && lda >= c_in && ldz >= c_out && lda % 4 == 0 && ldz % 4 == 0 &&
           packed && !(reinterpret_cast<uintptr_t>(packed) & 15) && rows >= 2 && rows <= M;
}

extern "C" int dal3_tr_linear_bn_stats(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                       int relu_in, const float* W, int64_t ldw, const float* bias, int64_t seg, int c_out,
                                       float* z, int64_t ldz, const void* packed, int64_t rows, const float* gamma,
                                       const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                                       float* mu, float* rstd, float* bn_scale, float* bn_shift, void* workspace,
                                       size_t workspace_bytes, dal3_stream stream) {
    if (!tr_linear_red_args_ok(a, M, c_in, lda, c_out, z, ldz, packed, rows) || !W || (scale && !shift) || seg < 0 || !gamma ||
        !beta || !mu || !rstd || !bn_scale || !bn_shift || (!running_mean != !running_var))
        return fail(DAL3_EINVAL, "tr_linear_bn_stats: bad argument");
    if (tr_linear_pack_mtb(M, c_in, seg, c_out, 0, scale != nullptr) == 0)
        return fail(DAL3_EINVAL, "tr_linear_bn_stats: this call reads no packed image (dal3_tr_linear_pack_layout() == 0)");
    if (!workspace || workspace_bytes < dal3_tr_linear_red_workspace_bytes(rows, c_out))
        return fail(DAL3_EWORKSPACE, "tr_linear_bn_stats: workspace smaller than dal3_tr_linear_red_workspace_bytes()");
    int fused = 0;
    HIP_TRY(launch_tr_linear_bn_stats(a, M, c_in, lda, scale, shift, relu_in, W, ldw, bias, seg, c_out, z, ldz,
                                      const_cast<float*>(static_cast<const float*>(packed)), rows, gamma, beta, running_mean,
                                      running_var, momentum, eps, mu, rstd, bn_scale, bn_shift, static_cast<double*>(workspace),
                                      static_cast<hipStream_t>(stream), &fused));
    return fused;
}

extern "C" int dal3_tr_linear_bnbwd_sums(const float* dz, int64_t M, int c_in, int64_t lddz, const float* W, int64_t ldw, int c_out,
                                         float* da, int64_t ldda, const void* packed, int64_t rows, const float* bz, int64_t ldbz,
                                         const float* bscale, const float* bshift, const float* bmu, const float* brstd,
                                         const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2, float* k3,
                                         void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!tr_linear_red_args_ok(dz, M, c_in, lddz, c_out, da, ldda, packed, rows) || !W || !bz || ldbz < c_out || ldbz % 4 ||
        !bscale || !bshift || !bmu || !brstd || !gamma || !dgamma || !dbeta || !k1 || !k2 || !k3)
        return fail(DAL3_EINVAL, "tr_linear_bnbwd_sums: bad argument");
    if (tr_linear_pack_mtb(M, c_in, 0, c_out, 0, 0) == 0)
        return fail(DAL3_EINVAL, "tr_linear_bnbwd_sums: this call reads no packed image (dal3_tr_linear_pack_layout() == 0)");
    if (!workspace || workspace_bytes < dal3_tr_linear_red_workspace_bytes(rows, c_out))
        return fail(DAL3_EWORKSPACE, "tr_linear_bnbwd_sums: workspace smaller than dal3_tr_linear_red_workspace_bytes()");
    int fused = 0;
    HIP_TRY(launch_tr_linear_bnbwd_sums(dz, M, c_in, lddz, W, ldw, c_out, da, ldda, const_cast<float*>(static_cast<const float*>(packed)),
                                        rows, bz, ldbz, bscale, bshift, bmu, brstd, gamma, dgamma, dbeta, k1, k2, k3,
                                        static_cast<double*>(workspace), static_cast<hipStream_t>(stream), &fused));
    return fused;
}

extern "C" int dal3_tr_linear_x3_layout(int64_t M, int c_in, int64_t seg, int c_out, int accumulate, int has_act) {
    if (!mult32(M) || !mult32(c_in) || !mult32(c_out)) return 0;
    return tr_linear_x3_layout(M, c_in, seg, c_out, accumulate, has_act);
}

extern "C" int dal3_tr_linear_x3(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                 int relu_in, const float* bias, int64_t seg, int c_out, float* z, int64_t ldz,
                                 const void* packed, const uint32_t* in_amax, dal3_stream stream) {
    if (!a || !z || !mult32(M) || !mult32(c_in) || !mult32(c_out) || lda < c_in || ldz < c_out || lda % 4 || ldz % 4 ||
        (scale && !shift) || seg < 0 || !packed || (reinterpret_cast<uintptr_t>(packed) & 15) || (in_amax && scale) ||
        (reinterpret_cast<uintptr_t>(in_amax) & 3) ||
        (reinterpret_cast<uintptr_t>(a) & 15) || (reinterpret_cast<uintptr_t>(z) & 15) || (bias && (reinterpret_cast<uintptr_t>(bias) & 15)))
        return fail(DAL3_EINVAL, "tr_linear_x3: bad argument (16-byte aligned a / z / bias / packed, row strides multiples of 4)");
    const int layout = tr_linear_x3_layout(M, c_in, seg, c_out, 0, scale != nullptr);
    if (layout == 0) return fail(DAL3_EINVAL, "tr_linear_x3: this shape does not take the f16x3 kernel (dal3_tr_linear_x3_layout() == 0)");
    if (lda * 64 * (int64_t)sizeof(float) >= ((int64_t)1 << 31)) return fail(DAL3_EINVAL, "tr_linear_x3: lda too large");
    HIP_TRY(launch_tr_linear_x3(a, M, c_in, lda, scale, shift, relu_in, static_cast<const uint16_t*>(packed), layout, bias, seg, c_out,
                                z, ldz, static_cast<hipStream_t>(stream), in_amax));
    return 0;
}

extern "C" size_t dal3_tr_linear_workspace_bytes(int c_in, int c_out) {
    return (c_in > 0 && c_out > 0) ? tr_linear_workspace_bytes(c_in, c_out) : 0;
}

extern "C" size_t dal3_tr_colred_workspace_bytes(int64_t M, int C) {
    return (M > 0 && C > 0) ? tr_colred_workspace_bytes(M, C) : 0;
}

extern "C" int dal3_tr_act_colsum(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift, int relu,
                                  float* out, int64_t ldo, void* workspace, size_t workspace_bytes, double* sums, dal3_stream stream) {
    if (!x || !out || !sums || M <= 0 || C <= 0 || (C & 3) || ldx < C || (ldx & 3) || ldo < C || (ldo & 3) || (scale && !shift))
        return fail(DAL3_EINVAL, "tr_act_colsum: bad argument (C and the row strides multiples of 4)");
    if (!workspace || workspace_bytes < tr_colred_workspace_bytes(M, C))
        return fail(DAL3_EWORKSPACE, "tr_act_colsum: workspace smaller than dal3_tr_colred_workspace_bytes()");
    HIP_TRY(launch_tr_act_colsum(x, M, C, ldx, scale, shift, relu, out, ldo, static_cast<double*>(workspace), sums,
                                 static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_colred(const float* z, int64_t M, int C, int64_t ldz, int mode, const float* da, int64_t ldda,
                              const float* dg, const int32_t* arg, int64_t seg, const float* scale, const float* shift,
                              const float* mu, const float* rstd, void* workspace, size_t workspace_bytes, double* out,
                              dal3_stream stream) {
    if (!z || M <= 0 || C <= 0 || C % 4 || ldz < C || ldz % 4 || !out || (mode != 0 && mode != 1) || (da && ldda % 4))
        return fail(DAL3_EINVAL, "tr_colred: bad argument (C and the row strides must be multiples of 4)");
    if (mode == 1 && (!scale || !shift || !mu || !rstd || (!da && (!dg || !arg || seg <= 0))))
        return fail(DAL3_EINVAL, "tr_colred: mode 1 needs scale/shift/mu/rstd and da or (dg, arg, seg)");
    if (!workspace || workspace_bytes < tr_colred_workspace_bytes(M, C))
        return fail(DAL3_EWORKSPACE, "tr_colred: workspace smaller than dal3_tr_colred_workspace_bytes()");
    HIP_TRY(launch_tr_colred(z, M, C, ldz, mode, da, ldda, dg, arg, seg, scale, shift, mu, rstd,
                             static_cast<double*>(workspace), out, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_pool_coef(const float* dg, const float* g, const float* zarg, const float* mu, const float* rstd,
                                 const float* gamma, int B, int C, int64_t M, double* coef, float* kd, dal3_stream stream) {
    if (!dg || !g || !zarg || !mu || !rstd || !gamma || B <= 0 || C <= 0 || M <= 0 || !coef || !kd)
        return fail(DAL3_EINVAL, "tr_pool_coef: bad argument");
    HIP_TRY(launch_tr_pool_coef(dg, g, zarg, mu, rstd, gamma, B, C, M, coef, kd, static_cast<hipStream_t>(stream)));
    return 0;
}


extern "C" int dal3_tr_pool_moments(const float* W, int64_t ldw, const float* b, const double* m1, const float* Sc, int64_t M, int C,
                                    int K, double* sums, dal3_stream stream) {
    if (!W || !b || !m1 || !Sc || !sums || M <= 0 || C <= 0 || !tr_pool_k_ok(K) || ldw < K)
        return fail(DAL3_EINVAL, "tr_pool_moments: bad argument (K = 64, 128 or 256; ldw >= K)");
    HIP_TRY(launch_tr_pool_moments(W, ldw, b, m1, Sc, M, C, K, sums, static_cast<hipStream_t>(stream)));
    return 0;
}


extern "C" size_t dal3_tr_conv1_workspace_bytes(int64_t Mp, int c_out) { return Mp > 0 && c_out > 0 ? tr_conv1_workspace_bytes(Mp, c_out) : 0; }

extern "C" int dal3_tr_conv1_bn_stats(const float* x, int64_t M, int64_t Mp, int c_in, int64_t ldx, const float* W, int64_t ldw,
                                      const float* bias, int c_out, float* z, int64_t ldz, const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                      float* scale, float* shift, void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!x || !W || !bias || !z || !gamma || !beta || !mu || !rstd || !scale || !shift || M < 2 || Mp < M || !tr_conv1_ok(c_in, c_out) ||
        ldx < c_in || ldw < c_in || ldz < c_out || (ldz & 3) || (!running_mean != !running_var) ||
        (reinterpret_cast<uintptr_t>(z) & 15) || (reinterpret_cast<uintptr_t>(bias) & 15))
        return fail(DAL3_EINVAL, "tr_conv1_bn_stats: bad argument (c_in <= 8, c_out 64 or 128, 16-byte aligned z / bias, M >= 2)");
    if (!workspace || workspace_bytes < tr_conv1_workspace_bytes(Mp, c_out))
        return fail(DAL3_EWORKSPACE, "tr_conv1_bn_stats: workspace smaller than dal3_tr_conv1_workspace_bytes()");
    HIP_TRY(launch_tr_conv1_bn_stats(x, M, Mp, c_in, ldx, W, ldw, bias, c_out, z, ldz, gamma, beta, running_mean, running_var, momentum,
                                     eps, mu, rstd, scale, shift, static_cast<double*>(workspace), static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_conv1_wgrad(const float* dz, int64_t lddz, const float* x, int64_t M, int c_in, int64_t ldx, int c_out,
                                   void* workspace, size_t workspace_bytes, float* dW, dal3_stream stream) {
    if (!dz || !x || !dW || M <= 0 || !tr_conv1_ok(c_in, c_out) || ldx < c_in || lddz < c_out || (lddz & 3) ||
        (reinterpret_cast<uintptr_t>(dz) & 15))
        return fail(DAL3_EINVAL, "tr_conv1_wgrad: bad argument (c_in <= 8, c_out 64 or 128, 16-byte aligned dz)");
    if (!workspace || workspace_bytes < tr_conv1_workspace_bytes(M, c_out))
        return fail(DAL3_EWORKSPACE, "tr_conv1_wgrad: workspace smaller than dal3_tr_conv1_workspace_bytes()");
    HIP_TRY(launch_tr_conv1_wgrad(dz, lddz, x, M, c_in, ldx, c_out, static_cast<double*>(workspace), dW, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_parse_box_pred(const float* box_pred, int64_t ldb, int64_t B, float* center, float* heading_scores,
                                   float* heading_residuals_normalized, float* heading_residuals, float* size_scores,
                                   float* size_residuals_normalized, float* size_residuals, dal3_stream stream) {
    if (!box_pred || !center || !heading_scores || !heading_residuals_normalized || !heading_residuals || !size_scores ||
        !size_residuals_normalized || !size_residuals || B <= 0 || B > (1 << 24) || ldb < 39)
        return fail(DAL3_EINVAL, "parse_box_pred: bad argument (seven outputs, ldb >= 39)");
    HIP_TRY(launch_parse_box_pred(box_pred, ldb, (int)B, center, heading_scores, heading_residuals_normalized, heading_residuals,
                                  size_scores, size_residuals_normalized, size_residuals, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_parse_box_pred_backward(const float* g_center, const float* g_heading_scores,
                                            const float* g_heading_residuals_normalized, const float* g_heading_residuals,
                                            const float* g_size_scores, const float* g_size_residuals_normalized,
                                            const float* g_size_residuals, int64_t B, float* g_box_pred, dal3_stream stream) {
    if (!g_box_pred || B <= 0 || B > (1 << 24)) return fail(DAL3_EINVAL, "parse_box_pred_backward: bad argument");
    HIP_TRY(launch_parse_box_pred_backward(g_center, g_heading_scores, g_heading_residuals_normalized, g_heading_residuals, g_size_scores,
                                           g_size_residuals_normalized, g_size_residuals, (int)B, g_box_pred,
                                           static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_fc_max_rows(void) { return tr_fc_max_rows(); }
extern "C" int dal3_tr_fc_max_act_cin(void) { return tr_fc_max_act_cin(); }

extern "C" int dal3_tr_fc_forward(const float* a, int64_t B, int c_in, int64_t lda, const float* in_scale, const float* in_shift,
                                  int relu_in, const float* W, int64_t ldw, int transpose_w, const float* bias, int c_out, float* z,
                                  int64_t ldz, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                  float momentum, float eps, float* mu, float* rstd, float* scale, float* shift, dal3_stream stream) {
    if (!a || !W || !z || B < 1 || B > tr_fc_max_rows() || c_in <= 0 || c_out <= 0 || lda < c_in || ldz < c_out ||
        ldw < (transpose_w ? c_out : c_in) || (in_scale && (!in_shift || c_in > tr_fc_max_act_cin())) || (!running_mean != !running_var))
        return fail(DAL3_EINVAL, "tr_fc_forward: bad argument (1 <= B <= dal3_tr_fc_max_rows(); strides at least the row lengths; "
                                 "c_in <= 2048 under an input activation)");
    if (gamma && (!beta || !mu || !rstd || !scale || !shift || B < 2))
        return fail(DAL3_EINVAL, "tr_fc_forward: a BatchNorm needs beta, the four outputs and at least two rows");
    HIP_TRY(launch_tr_fc_forward(a, (int)B, c_in, lda, in_scale, in_shift, relu_in, W, ldw, transpose_w, bias, c_out, z, ldz, gamma, beta,
                                 gamma ? running_mean : nullptr, gamma ? running_var : nullptr, momentum, eps, mu, rstd, scale, shift,
                                 static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_fc_backward_w(const float* da, int64_t ldda, int64_t B, int c_out, const float* z, int64_t ldz, const float* scale,
                                     const float* shift, const float* mu, const float* rstd, const float* gamma, float* dgamma,
                                     float* dbeta, const float* a_prev, int c_in, int64_t lda, const float* in_scale,
                                     const float* in_shift, int relu_in, float* dz, int64_t lddz, float* dW, int64_t lddw, float* db,
                                     dal3_stream stream) {
    if (!da || B < 1 || B > tr_fc_max_rows() || c_out <= 0 || ldda < c_out || (dz && lddz < c_out) ||
        (in_scale && (!in_shift || c_in > tr_fc_max_act_cin())) ||
        (dW && (!a_prev || c_in <= 0 || lda < c_in || lddw < c_in)))
        return fail(DAL3_EINVAL, "tr_fc_backward_w: bad argument (1 <= B <= dal3_tr_fc_max_rows(); strides at least the row lengths)");
    if (scale && (!z || ldz < c_out || !shift || !mu || !rstd || !gamma || !dgamma || !dbeta))
        return fail(DAL3_EINVAL, "tr_fc_backward_w: a BatchNorm needs z, shift, mu, rstd, gamma and the two gradient outputs");
    HIP_TRY(launch_tr_fc_backward_w(da, ldda, (int)B, c_out, z, ldz, scale, shift, mu, rstd, gamma, dgamma, dbeta, a_prev, c_in, lda,
                                    in_scale, in_shift, relu_in, dz, lddz, dW, lddw, db, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_gather_at(const float* z, int64_t ldz, const int32_t* arg, int64_t seg, int n_seg, int C, float* out,
                                 dal3_stream stream) {
    if (!z || !arg || !out || seg <= 0 || n_seg <= 0 || C <= 0 || ldz < C) return fail(DAL3_EINVAL, "tr_gather_at: bad argument");
    HIP_TRY(launch_tr_gather_at(z, ldz, arg, seg, n_seg, C, out, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_pool_zarg(const int32_t* arg, const float* a, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                 int B, int C, int K, int N, float* zarg, dal3_stream stream) {
    if (!arg || !a || !W || !bias || !zarg || B <= 0 || C <= 0 || N <= 0 || K <= 0 || K % 4 || lda < K || ldw < K || lda % 4 || ldw % 4 ||
        (reinterpret_cast<uintptr_t>(a) & 15) || (reinterpret_cast<uintptr_t>(W) & 15))
        return fail(DAL3_EINVAL, "tr_pool_zarg: bad argument (K and the row strides multiples of 4, 16-byte aligned a / W)");
    HIP_TRY(launch_tr_pool_zarg(arg, a, lda, W, ldw, bias, B, C, K, N, zarg, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_tr_pool_gv_workspace_bytes(int K) { return tr_pool_k_ok(K) ? tr_pool_gv_workspace_bytes(K) : 0; }

extern "C" int dal3_tr_pool_gv(const double* coef, const float* W, int64_t ldw, const float* b, int C, int K, float* G, float* v,
                               void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!coef || !W || !b || !G || !v || C <= 0 || !tr_pool_k_ok(K) || ldw < K)
        return fail(DAL3_EINVAL, "tr_pool_gv: bad argument (K = 64, 128 or 256; ldw >= K)");
    if (!workspace || workspace_bytes < tr_pool_gv_workspace_bytes(K))
        return fail(DAL3_EWORKSPACE, "tr_pool_gv: workspace too small (dal3_tr_pool_gv_workspace_bytes)");
    HIP_TRY(launch_tr_pool_gv(coef, W, ldw, b, C, K, G, v, static_cast<double*>(workspace), static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_pool_dw(const double* coef, const float* W, int64_t ldw, const float* b, const float* S, const double* m1,
                               int64_t M, int centred, const float* dWs, int C, int K, float* dW, dal3_stream stream) {
    if (!coef || !W || !b || !S || !m1 || !dWs || !dW || M <= 0 || C <= 0 || !tr_pool_k_ok(K) || ldw < K)
        return fail(DAL3_EINVAL, "tr_pool_dw: bad argument (K = 64, 128 or 256; ldw >= K)");
    HIP_TRY(launch_tr_pool_dw(coef, W, ldw, b, S, m1, M, centred, dWs, C, K, dW, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_pool_sparse(const int32_t* arg, const float* kd, const float* W, int64_t ldw, const float* a,
                                   int64_t lda, int B, int C, int K, int N, float* da, int64_t ldda, float* dWs,
                                   dal3_stream stream) {
    if (!arg || !kd || !W || !a || !da || !dWs || B <= 0 || C <= 0 || N <= 0 || (K != 128 && K != 256 && K != 64) ||
        ldw < K || lda < K || ldda < K || ldw % 4 || ldda % 4)
        return fail(DAL3_EINVAL, "tr_pool_sparse: bad argument (K = 64, 128 or 256; row strides >= K, multiples of 4)");
    if ((size_t)(2 * (size_t)N + 1 + (size_t)C) * sizeof(int) > 65536 || C > 4096)
        return fail(DAL3_EINVAL, "tr_pool_sparse: 2 N + C + 1 must not exceed 16384 and C must not exceed 4096 (an item's buckets live in LDS)");
    HIP_TRY(launch_tr_pool_sparse(arg, kd, W, ldw, a, lda, B, C, K, N, da, ldda, dWs, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_box_loss(const float* center, const float* center_label, const float* heading_scores,
                                const float* heading_residuals_normalized, const int64_t* heading_class_label,
                                const float* heading_residuals_label, const float* size_scores,
                                const float* size_residuals_normalized, const int64_t* size_class_label,
                                const float* size_residuals_label, int B, float* losses, float* g_center,
                                float* g_heading_scores, float* g_heading_residuals_normalized, float* g_size_scores,
                                float* g_size_residuals_normalized, dal3_stream stream) {
    if (!center || !center_label || !heading_scores || !heading_residuals_normalized || !heading_class_label ||
        !heading_residuals_label || !size_scores || !size_residuals_normalized || !size_class_label ||
        !size_residuals_label || B <= 0 || !losses || !g_center || !g_heading_scores || !g_heading_residuals_normalized ||
        !g_size_scores || !g_size_residuals_normalized)
        return fail(DAL3_EINVAL, "tr_box_loss: bad argument");
    HIP_TRY(launch_tr_box_loss(center, center_label, heading_scores, heading_residuals_normalized, heading_class_label,
                               heading_residuals_label, size_scores, size_residuals_normalized, size_class_label,
                               size_residuals_label, B, losses, g_center, g_heading_scores, g_heading_residuals_normalized,
                               g_size_scores, g_size_residuals_normalized, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_tr_seg_ce_workspace_bytes(int64_t M) { return M > 0 ? tr_seg_ce_workspace_bytes(M) : 0; }

extern "C" int dal3_tr_seg_ce(const float* logits, const void* labels, int labels_are_int64, int64_t M, float* loss,
                              float* dlogits, void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!logits || !labels || M <= 0 || !loss || !dlogits) return fail(DAL3_EINVAL, "tr_seg_ce: bad argument");
    if ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits)) & 7)
        return fail(DAL3_EINVAL, "tr_seg_ce: logits and dlogits must be 8-byte aligned");
    if (!workspace || workspace_bytes < tr_seg_ce_workspace_bytes(M) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(DAL3_EWORKSPACE, "tr_seg_ce: workspace smaller than dal3_tr_seg_ce_workspace_bytes() or misaligned");
    HIP_TRY(launch_tr_seg_ce(logits, labels, labels_are_int64, M, loss, dlogits, static_cast<double*>(workspace),
                             static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_bn_stats(const float* z, int64_t M, int C, int64_t ldz, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, float momentum, float eps, float* mu, float* rstd,
                                float* scale, float* shift, void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!z || M < 2 || C <= 0 || C % 4 || ldz < C || ldz % 4 || !gamma || !beta || !mu || !rstd || !scale || !shift ||
        (!running_mean != !running_var))
        return fail(DAL3_EINVAL, "tr_bn_stats: bad argument (C and the row stride must be multiples of 4, M >= 2)");
    if (!workspace || workspace_bytes < tr_colred_workspace_bytes(M, C))
        return fail(DAL3_EWORKSPACE, "tr_bn_stats: workspace smaller than dal3_tr_colred_workspace_bytes()");
    HIP_TRY(launch_tr_bn_stats(z, M, C, ldz, gamma, beta, running_mean, running_var, momentum, eps, mu, rstd, scale, shift,
                               static_cast<double*>(workspace), static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_bnbwd_sums(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                  const float* dg, const int32_t* arg, int64_t seg, const float* scale, const float* shift,
                                  const float* mu, const float* rstd, const float* gamma, float* dgamma, float* dbeta,
                                  float* k1, float* k2, float* k3, void* workspace, size_t workspace_bytes,
                                  dal3_stream stream) {
    if (!z || M <= 0 || C <= 0 || C % 4 || ldz < C || ldz % 4 || (da && ldda % 4) || !scale || !shift || !mu || !rstd ||
        (!da && (!dg || !arg || seg <= 0)) || !gamma || !dgamma || !dbeta || !k1 || !k2 || !k3)
        return fail(DAL3_EINVAL, "tr_bnbwd_sums: bad argument (C and the row strides must be multiples of 4)");
    if (!workspace || workspace_bytes < tr_colred_workspace_bytes(M, C))
        return fail(DAL3_EWORKSPACE, "tr_bnbwd_sums: workspace smaller than dal3_tr_colred_workspace_bytes()");
    HIP_TRY(launch_tr_bnbwd_sums(z, M, C, ldz, da, ldda, dg, arg, seg, scale, shift, mu, rstd, gamma, dgamma, dbeta, k1, k2,
                                 k3, static_cast<double*>(workspace), static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_bn_finalize(const double* sums, int C, int64_t M, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, float momentum, float eps, float* mu,
                                   float* rstd, float* scale, float* shift, dal3_stream stream) {
    if (!sums || C <= 0 || M < 2 || !gamma || !beta || !mu || !rstd || !scale || !shift || (!running_mean != !running_var))
        return fail(DAL3_EINVAL, "tr_bn_finalize: bad argument");
    HIP_TRY(launch_tr_bn_finalize(sums, C, M, gamma, beta, running_mean, running_var, momentum, eps, mu, rstd, scale, shift,
                                  static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_bnbwd_coef(const double* sums, int C, int64_t M, const float* gamma, const float* rstd, float* dgamma,
                                  float* dbeta, float* k1, float* k2, float* k3, dal3_stream stream) {
    if (!sums || C <= 0 || M <= 0 || !gamma || !rstd || !dgamma || !dbeta || !k1 || !k2 || !k3)
        return fail(DAL3_EINVAL, "tr_bnbwd_coef: bad argument");
    HIP_TRY(launch_tr_bnbwd_coef(sums, C, M, gamma, rstd, dgamma, dbeta, k1, k2, k3, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_bnbwd_apply(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                   const float* dg, const int32_t* arg, int64_t seg, const float* scale,
                                   const float* shift, const float* mu, const float* rstd, const float* k1,
                                   const float* k2, const float* k3, float* dz, int64_t lddz, dal3_stream stream) {
    if (!z || M <= 0 || C <= 0 || C % 4 || !scale || !shift || !mu || !rstd || !k1 || !k2 || !k3 || !dz || ldz < C ||
        lddz < C || ldz % 4 || lddz % 4 || (da && ldda % 4) || (!da && (!dg || !arg || seg <= 0)))
        return fail(DAL3_EINVAL, "tr_bnbwd_apply: bad argument (C and the row strides must be multiples of 4)");
    HIP_TRY(launch_tr_bnbwd_apply(z, M, C, ldz, da, ldda, dg, arg, seg, scale, shift, mu, rstd, k1, k2, k3, dz, lddz,
                                  static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_bnbwd_apply_amax(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                        const float* dg, const int32_t* arg, int64_t seg, const float* scale,
                                        const float* shift, const float* mu, const float* rstd, const float* k1,
                                        const float* k2, const float* k3, float* dz, int64_t lddz, uint32_t* amax,
                                        dal3_stream stream) {
    if (!z || M <= 0 || C <= 0 || C % 64 || !scale || !shift || !mu || !rstd || !k1 || !k2 || !k3 || !dz || ldz < C ||
        lddz < C || ldz % 4 || lddz % 4 || (da && ldda % 4) || (!da && (!dg || !arg || seg <= 0)) || !amax ||
        (reinterpret_cast<uintptr_t>(amax) & 3))
        return fail(DAL3_EINVAL, "tr_bnbwd_apply_amax: bad argument (C a multiple of 64, the row strides of 4, amax 64 device words)");
    HIP_TRY(launch_tr_bnbwd_apply(z, M, C, ldz, da, ldda, dg, arg, seg, scale, shift, mu, rstd, k1, k2, k3, dz, lddz,
                                  static_cast<hipStream_t>(stream), amax));
    return 0;
}

extern "C" size_t dal3_tr_bnbwd_apply_segsum_workspace_bytes(int64_t M, int C) {
    return (M > 0 && C > 0) ? tr_bnbwd_apply_segsum_workspace_bytes(M, C) : 0;
}

extern "C" int dal3_tr_bnbwd_apply_segsum(const float* z, int64_t M, int C, int64_t ldz, const float* da, int64_t ldda,
                                          const float* scale, const float* shift, const float* mu, const float* rstd,
                                          const float* k1, const float* k2, const float* k3, float* dz, int64_t lddz,
                                          int64_t sum_seg, float* seg_sums, void* workspace, size_t workspace_bytes,
                                          dal3_stream stream) {
    if (!z || !da || M <= 0 || C <= 0 || C % 64 || !scale || !shift || !mu || !rstd || !k1 || !k2 || !k3 || !dz || ldz < C ||
        lddz < C || ldda < C || ldz % 4 || lddz % 4 || ldda % 4 || sum_seg <= 0 || sum_seg % 128 || M % sum_seg || !seg_sums)
        return fail(DAL3_EINVAL, "tr_bnbwd_apply_segsum: bad argument (C % 64 == 0, sum_seg % 128 == 0, M % sum_seg == 0, dense da)");
    if (!workspace || workspace_bytes < tr_bnbwd_apply_segsum_workspace_bytes(M, C))
        return fail(DAL3_EWORKSPACE, "tr_bnbwd_apply_segsum: workspace too small");
    HIP_TRY(launch_tr_bnbwd_apply_segsum(z, M, C, ldz, da, ldda, scale, shift, mu, rstd, k1, k2, k3, dz, lddz, sum_seg, seg_sums,
                                         static_cast<double*>(workspace), static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_tr_wgrad_workspace_bytes(int64_t M, int c_out, int c_in) {
    return (M > 0 && c_out > 0 && c_in > 0) ? tr_wgrad_workspace_bytes(M, c_out, c_in) : 0;
}

extern "C" int dal3_tr_wgrad(const float* dz, int64_t lddz, const float* a, int64_t lda, const float* scale,
                             const float* shift, int relu_in, int64_t M, int c_out, int c_in, void* workspace,
                             size_t workspace_bytes, float* dW, dal3_stream stream) {
    if (!dz || !a || !mult32(M) || !mult32(c_out) || !mult32(c_in) || lddz < c_out || lda < c_in || (scale && !shift))
        return fail(DAL3_EINVAL, "tr_wgrad: bad argument (M, c_in, c_out multiples of 32)");
    if (!workspace || workspace_bytes < tr_wgrad_workspace_bytes(M, c_out, c_in))
        return fail(DAL3_EWORKSPACE, "tr_wgrad: workspace smaller than dal3_tr_wgrad_workspace_bytes()");
    HIP_TRY(launch_tr_wgrad(dz, lddz, a, lda, scale, shift, relu_in, M, c_out, c_in, static_cast<float*>(workspace), dW,
                            static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_wgrad_final_many(const dal3_tr_wgrad_part* items, int n, dal3_stream stream) {
    if (!items || n <= 0 || n > 24) return fail(DAL3_EINVAL, "tr_wgrad_final_many: 1 .. 24 items");
    for (int i = 0; i < n; ++i)
        if (!items[i].part || !items[i].dW || items[i].n <= 0 || items[i].n_slices <= 0 || items[i].n_slices > 0x7fffffff)
            return fail(DAL3_EINVAL, "tr_wgrad_final_many: bad item %d", i);
    HIP_TRY(launch_tr_wgrad_final_many(items, n, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_tr_wgrad_x3_workspace_bytes(int64_t M, int c_out, int c_in) {
    return (M > 0 && c_out > 0 && c_in > 0 && tr_wgrad_x3_ok(M, c_out, c_in)) ? tr_wgrad_x3_workspace_bytes(M, c_out, c_in) : 0;
}

extern "C" int dal3_tr_wgrad_x3(const float* dz, int64_t lddz, const float* a, int64_t lda, const float* scale,
                                const float* shift, int relu_in, const uint32_t* dz_amax, int64_t M, int c_out, int c_in,
                                void* workspace, size_t workspace_bytes, float* dW, dal3_stream stream) {
    if (!dz || !a || !mult32(M) || !mult32(c_out) || !mult32(c_in) || lddz < c_out || lda < c_in || (scale && !shift) ||
        (lddz & 3) || (lda & 3) || (reinterpret_cast<uintptr_t>(dz) & 15) || (reinterpret_cast<uintptr_t>(a) & 15) ||
        (scale && ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 15)) ||
        (reinterpret_cast<uintptr_t>(dz_amax) & 3))
        return fail(DAL3_EINVAL, "tr_wgrad_x3: bad argument (M, c_in, c_out multiples of 32; 16-byte aligned operands, strides multiples of 4)");
    if (!tr_wgrad_x3_ok(M, c_out, c_in))
        return fail(DAL3_EINVAL, "tr_wgrad_x3: this shape does not take the f16x3 kernel (dal3_tr_wgrad_x3_workspace_bytes() == 0)");
    if (!workspace || workspace_bytes < tr_wgrad_x3_workspace_bytes(M, c_out, c_in))
        return fail(DAL3_EWORKSPACE, "tr_wgrad_x3: workspace smaller than dal3_tr_wgrad_x3_workspace_bytes()");
    HIP_TRY(launch_tr_wgrad_x3(dz, lddz, a, lda, scale, shift, relu_in, dz_amax, M, c_out, c_in, static_cast<float*>(workspace), dW,
                               static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_segmax(const float* z, int64_t ldz, int64_t seg, int C, const float* scale, const float* shift,
                              float* g, int32_t* arg, int64_t n_seg, void* workspace, size_t workspace_bytes,
                              dal3_stream stream) {
    if (!z || !scale || !shift || !g || !arg || seg <= 0 || C <= 0 || n_seg <= 0 || ldz < C)
        return fail(DAL3_EINVAL, "tr_segmax: bad argument");
    if (!workspace || workspace_bytes < (size_t)n_seg * C * 8 || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(DAL3_EWORKSPACE, "tr_segmax: workspace needs n_seg * C * 8 bytes, 8-byte aligned");
    HIP_TRY(launch_tr_segmax(z, ldz, seg, C, scale, shift, g, arg, n_seg, static_cast<unsigned long long*>(workspace),
                             static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_act_dropout(const float* x, int64_t M, int C, int64_t ldx, const float* scale, const float* shift,
                                   int relu, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop,
                                   float* out, int64_t ldo, dal3_stream stream) {
    if (!x || !out || M <= 0 || C <= 0 || (C & 3) || ldx < C || ldo < C || (ldx & 3) || (ldo & 3) || (scale && !shift) ||
        (mult && (ldm < C || (ldm & 3))) || !(p_drop >= 0.0f && p_drop <= 1.0f))
        return fail(DAL3_EINVAL, "tr_act_dropout: bad argument (C and the row strides multiples of 4, 0 <= p <= 1)");
    HIP_TRY(launch_tr_act_dropout(x, M, C, ldx, scale, shift, relu, mult, ldm, seed, step, p_drop, out, ldo,
                                  static_cast<hipStream_t>(stream)));
    return 0;
}

static bool head2_common_ok(int64_t M, int C, const float* mult, int64_t ldm, float p_drop) {
    return M > 0 && C == 128 && (!mult || (ldm >= C && !(ldm & 3) && !(reinterpret_cast<uintptr_t>(mult) & 15))) &&
           p_drop >= 0.0f && p_drop <= 1.0f;
}

extern "C" int dal3_tr_head2_forward(const float* z, int64_t M, int C, int64_t ldz, const float* scale, const float* shift, int relu,
                                     const float* mult, int64_t ldm, uint64_t seed, const int64_t* step, float p_drop,
                                     const float* W, int64_t ldw, const float* bias, float* logits, dal3_stream stream) {
    if (!z || !W || !bias || !logits || !head2_common_ok(M, C, mult, ldm, p_drop) || ldz < C || (ldz & 3) || ldw < C || (ldw & 3) ||
        (scale && !shift) || (reinterpret_cast<uintptr_t>(z) & 15) || (reinterpret_cast<uintptr_t>(W) & 15) ||
        (reinterpret_cast<uintptr_t>(logits) & 7))
        return fail(DAL3_EINVAL, "tr_head2_forward: bad argument (C == 128, row strides multiples of 4, 16-byte aligned z / W / mult)");
    HIP_TRY(launch_tr_head2_forward(z, M, ldz, scale, shift, relu, mult, ldm, seed, step, p_drop, W, ldw, bias, logits,
                                    static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_head2_dgrad(const float* dlogits, int64_t M, int C, const float* mult, int64_t ldm, uint64_t seed,
                                   const int64_t* step, float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda,
                                   dal3_stream stream) {
    if (!dlogits || !W || !da || !head2_common_ok(M, C, mult, ldm, p_drop) || ldw < C || (ldw & 3) || ldda < C || (ldda & 3) ||
        (reinterpret_cast<uintptr_t>(dlogits) & 7) || (reinterpret_cast<uintptr_t>(W) & 15) || (reinterpret_cast<uintptr_t>(da) & 15))
        return fail(DAL3_EINVAL, "tr_head2_dgrad: bad argument (C == 128, row strides multiples of 4, aligned pointers)");
    HIP_TRY(launch_tr_head2_dgrad(dlogits, M, mult, ldm, seed, step, p_drop, W, ldw, da, ldda, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_head2_dgrad_bnbwd(const float* dlogits, int64_t M, int C, const float* mult, int64_t ldm, uint64_t seed,
                                         const int64_t* step, float p_drop, const float* W, int64_t ldw, float* da, int64_t ldda,
                                         const float* bz, int64_t ldbz, const float* bscale, const float* bshift, const float* bmu,
                                         const float* brstd, const float* gamma, float* dgamma, float* dbeta, float* k1, float* k2,
                                         float* k3, void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!dlogits || !W || !da || !bz || !bscale || !bshift || !bmu || !brstd || !gamma || !dgamma || !dbeta || !k1 || !k2 || !k3 ||
        !head2_common_ok(M, C, mult, ldm, p_drop) || ldw < C || (ldw & 3) || ldda < C || (ldda & 3) || ldbz < C || (ldbz & 3) ||
        (reinterpret_cast<uintptr_t>(dlogits) & 7) || (reinterpret_cast<uintptr_t>(W) & 15) || (reinterpret_cast<uintptr_t>(da) & 15) ||
        (reinterpret_cast<uintptr_t>(bz) & 15))
        return fail(DAL3_EINVAL, "tr_head2_dgrad_bnbwd: bad argument (C == 128, row strides multiples of 4, aligned pointers)");
    if (!workspace || workspace_bytes < tr_colred_workspace_bytes(M, C))
        return fail(DAL3_EWORKSPACE, "tr_head2_dgrad_bnbwd: workspace smaller than dal3_tr_colred_workspace_bytes(M, 128)");
    HIP_TRY(launch_tr_head2_dgrad_bnbwd(dlogits, M, mult, ldm, seed, step, p_drop, W, ldw, da, ldda, bz, ldbz, bscale, bshift, bmu, brstd,
                                        gamma, dgamma, dbeta, k1, k2, k3, static_cast<double*>(workspace),
                                        static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_tr_head2_wgrad_workspace_bytes(int64_t M) { return M > 0 ? tr_head2_wgrad_workspace_bytes(M) : 0; }

extern "C" int dal3_tr_head2_wgrad(const float* dlogits, const float* z, int64_t M, int C, int64_t ldz, const float* scale,
                                   const float* shift, int relu, const float* mult, int64_t ldm, uint64_t seed, const int64_t* step,
                                   float p_drop, void* workspace, size_t workspace_bytes, float* dWb, dal3_stream stream) {
    if (!dlogits || !z || !dWb || !head2_common_ok(M, C, mult, ldm, p_drop) || ldz < C || (ldz & 3) || (scale && !shift) ||
        (reinterpret_cast<uintptr_t>(z) & 15) || (reinterpret_cast<uintptr_t>(dlogits) & 7))
        return fail(DAL3_EINVAL, "tr_head2_wgrad: bad argument (C == 128, row strides multiples of 4, aligned pointers)");
    if (!workspace || workspace_bytes < tr_head2_wgrad_workspace_bytes(M))
        return fail(DAL3_EWORKSPACE, "tr_head2_wgrad: workspace smaller than dal3_tr_head2_wgrad_workspace_bytes()");
    HIP_TRY(launch_tr_head2_wgrad(dlogits, z, M, ldz, scale, shift, relu, mult, ldm, seed, step, p_drop,
                                  static_cast<double*>(workspace), dWb, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_tr_linear_pool_workspace_bytes(int c_in, int c_out, int64_t n_seg) {
    return tr_linear_workspace_bytes(c_in, c_out) + (size_t)n_seg * c_out * 8;
}

extern "C" int dal3_tr_linear_pool(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                   int relu_in, const float* W, int64_t ldw, const float* bias, const float* out_scale,
                                   const float* out_shift, int64_t seg, int c_out, float* g, int32_t* arg, void* workspace,
                                   size_t workspace_bytes, dal3_stream stream) {
    if (!a || !W || !out_scale || !out_shift || !g || !arg || !mult32(M) || !mult32(c_in) || c_out <= 0 || c_out % 128 != 0 ||
        lda < c_in || (lda & 3) || ldw < c_in || (ldw & 3) || (scale && !shift) || (scale && c_in > 1024) || seg <= 0 ||
        seg % 32 != 0 || M % seg != 0)
        return fail(DAL3_EINVAL, "tr_linear_pool: bad argument (M, c_in multiples of 32; c_out of 128; seg a multiple of 32 "
                                 "that divides M; strides multiples of 4)");
    const size_t wbytes = tr_linear_workspace_bytes(c_in, c_out), need = wbytes + (size_t)(M / seg) * c_out * 8;
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) || (wbytes & 7))
        return fail(DAL3_EWORKSPACE, "tr_linear_pool: workspace smaller than dal3_tr_linear_pool_workspace_bytes() or not 16-byte aligned");
    char* base = static_cast<char*>(workspace);
    HIP_TRY(launch_tr_linear_pool(a, M, c_in, lda, scale, shift, relu_in, W, ldw, bias, out_scale, out_shift, seg, c_out, g, arg,
                                  reinterpret_cast<float*>(base), reinterpret_cast<unsigned long long*>(base + wbytes),
                                  static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_linear_pool_x3_ok(int64_t M, int c_in, int64_t seg, int c_out) {
    return (mult32(M) && mult32(c_in) && c_out > 0 && seg > 0 && M % seg == 0 && tr_linear_pool_x3_ok(M, c_in, seg, c_out)) ? 1 : 0;
}

extern "C" int dal3_tr_linear_pool_x3(const float* a, int64_t M, int c_in, int64_t lda, const float* scale, const float* shift,
                                      int relu_in, const float* W, int64_t ldw, const float* bias, const float* out_scale,
                                      const float* out_shift, int64_t seg, int c_out, float* g, int32_t* arg, void* workspace,
                                      size_t workspace_bytes, dal3_stream stream) {
    if (!a || !W || !out_scale || !out_shift || !g || !arg || !mult32(M) || !mult32(c_in) || c_out <= 0 || lda < c_in || (lda & 3) ||
        ldw < c_in || (ldw & 3) || (scale && !shift) || seg <= 0 || M % seg != 0 || (reinterpret_cast<uintptr_t>(a) & 15) ||
        lda * 64 * (int64_t)sizeof(float) >= ((int64_t)1 << 31))
        return fail(DAL3_EINVAL, "tr_linear_pool_x3: bad argument");
    if (!tr_linear_pool_x3_ok(M, c_in, seg, c_out))
        return fail(DAL3_EINVAL, "tr_linear_pool_x3: this shape does not take the f16x3 kernel (dal3_tr_linear_pool_x3_ok() == 0)");
    const size_t wbytes = tr_linear_workspace_bytes(c_in, c_out), need = wbytes + (size_t)(M / seg) * c_out * 8;
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) || (wbytes & 7))
        return fail(DAL3_EWORKSPACE, "tr_linear_pool_x3: workspace smaller than dal3_tr_linear_pool_workspace_bytes() or not 16-byte aligned");
    char* base = static_cast<char*>(workspace);
    HIP_TRY(launch_tr_linear_pool_x3(a, M, c_in, lda, scale, shift, relu_in, W, ldw, bias, out_scale, out_shift, seg, c_out, g, arg,
                                     reinterpret_cast<float*>(base), reinterpret_cast<unsigned long long*>(base + wbytes),
                                     static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_tr_segsum(const float* x, int64_t ldx, int64_t seg, int C, float* out, int64_t n_seg,
                              dal3_stream stream) {
    if (!x || !out || seg <= 0 || C <= 0 || n_seg <= 0 || ldx < C) return fail(DAL3_EINVAL, "tr_segsum: bad argument");
    HIP_TRY(launch_tr_segsum(x, ldx, seg, C, out, n_seg, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_maxpool_n(const float* x, int64_t rows, int64_t n, float* out, dal3_stream stream) {
    if (!x || !out || rows <= 0 || n <= 0) return fail(DAL3_EINVAL, "maxpool_n: bad argument");
    HIP_TRY(launch_maxpool_n(x, DAL3_F32, rows, n, out, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_maxpool_n_dtype(const void* x, int dtype, int64_t rows, int64_t n, void* out, dal3_stream stream) {
    if (dtype != DAL3_F32 && dtype != DAL3_BF16 && dtype != DAL3_F16) return fail(DAL3_EINVAL, "maxpool_n: storage dtype %d", dtype);
    if (!x || !out || rows <= 0 || n <= 0) return fail(DAL3_EINVAL, "maxpool_n: bad argument");
    if (dtype != DAL3_F32 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 1))
        return fail(DAL3_EINVAL, "maxpool_n: 16-bit rows must be 2-byte aligned");
    HIP_TRY(launch_maxpool_n(x, dtype, rows, n, out, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_shared_mlp_layer_workspace_bytes(int c_in, int c_out) {
    const size_t mt = (size_t)(c_out + 31) / 32;
    const size_t w = c_in <= 8 ? mt * 4 * 64 : mt * (size_t)(c_in / 32) * 1024;
    return (al(w) + al(mt * 32)) * sizeof(float);
}

extern "C" int dal3_shared_mlp_layer(const dal3_layer* layer, int relu, dal3_bcn x, int B, int N, float* y,
                                     void* workspace, size_t workspace_bytes, dal3_stream stream) {
    if (!layer || !y || !workspace) return fail(DAL3_EINVAL, "shared_mlp_layer: bad argument");
    TRY(check_extent(B, N, "shared_mlp_layer"));
    TRY(check_bcn(x, "x"));
    if (x.dtype != DAL3_F32) return fail(DAL3_EINVAL, "shared_mlp_layer: the layer-wise test entry takes fp32 input only");
    const dal3_layer& L = *layer;
    if (L.c_out % 32 != 0) return fail(DAL3_EINVAL, "shared_mlp_layer: c_out must be a multiple of 32");
    const bool first = L.c_in <= 8;
    if (!first && L.c_in % 32 != 0) return fail(DAL3_EINVAL, "shared_mlp_layer: c_in must be <= 8 or a multiple of 32");
    TRY(check_layer(L, L.c_in, L.c_out, "layer"));
    const size_t need = dal3_shared_mlp_layer_workspace_bytes(L.c_in, L.c_out);
    if (workspace_bytes < need) return fail(DAL3_EWORKSPACE, "shared_mlp_layer: workspace needs %zu bytes", need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int mt = L.c_out / 32;
    const int ks = first ? (L.c_in + 1) / 2 : 0;
    const int kt = first ? 0 : L.c_in / 32;
    float* wbuf = static_cast<float*>(workspace);
    float* bbuf = wbuf + al(first ? (size_t)mt * 4 * 64 : (size_t)mt * kt * 1024);
    if (first) HIP_TRY(launch_pack_weight(L, PACK_FIRST, 0, L.c_in, mt, ks, wbuf, s));
    else HIP_TRY(launch_pack_weight(L, PACK_FRAG_MT_MAJOR, 0, L.c_in, mt, kt, wbuf, s));
    HIP_TRY(launch_pack_bias(L, bbuf, s));
    HIP_TRY(launch_generic_layer(reinterpret_cast<const f32x4*>(wbuf), wbuf, bbuf, kt, ks, mt, relu, to_bcn(x), L.c_in,
                                 B, N, y, s));
    return 0;
}

// ---------------------------------------------------------------------------------- static model
struct StaticWs { InsSegWs seg; int32_t* pos; float* obj; float* obj2; HeadWs head; };
static StaticWs carve_static(Carver& c, int B, int N, int two_stage) {
    StaticWs w;
    w.seg = carve_ins_seg(c, B);
    w.pos = c.take<int32_t>((size_t)B * N);
    w.obj = c.take<float>((size_t)B * 512 * 3);
    w.obj2 = two_stage ? c.take<float>((size_t)B * 512 * 3) : nullptr;
    w.head = carve_head(c, B);
    return w;
}
extern "C" size_t dal3_static_workspace_bytes(int B, int N, int two_stage) {
    Carver c(nullptr, 0);
    carve_static(c, B, N, two_stage);
    return c.off;
}

extern "C" int dal3_static_forward(const dal3_static_args* a, int phases, dal3_stream stream) {
    if (!a) return fail(DAL3_EINVAL, "static_forward: args is NULL");
    TRY(check_extent(a->B, a->N, "static_forward"));
    if (!a->workspace) return fail(DAL3_EINVAL, "static_forward: workspace is NULL");
    if (!(phases & DAL3_PHASE_ALL)) return fail(DAL3_EINVAL, "static_forward: no phase selected");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Carver c(a->workspace, a->workspace_bytes);
    const StaticWs ws = carve_static(c, a->B, a->N, a->two_stage);
    if (!c.ok) return fail(DAL3_EWORKSPACE, "static_forward: workspace needs %zu bytes, got %zu", c.off, a->workspace_bytes);
    const int B = a->B, N = a->N, M = 512;

    if (phases & DAL3_PHASE_SEG) {
        TRY(ins_seg_run(a->w_ins_seg, a->dtype, 3, a->pts, B, N, a->logits, a->mask, nullptr, ws.seg, s));
        // (when the box phase follows in this call, its compaction kernel writes the same counts)
        if (a->counts && !(phases & DAL3_PHASE_BOX)) HIP_TRY(launch_segment_counts(a->mask, B, N, a->counts, s));
    }
    if (!(phases & DAL3_PHASE_BOX)) return 0;

    if (!a->init_box || !a->box_pred_one || !a->counts || !a->obj_idx || !a->w_box_est_one)
        return fail(DAL3_EINVAL, "static_forward: null pointer in box phase");
    TRY(gather_run(a->mask, a->pts, B, N, 3, M, a->sampler, a->choice, a->seed, a->item_offset, a->counts, a->obj_idx,
                   ws.obj, ws.pos, s));
    const dal3_bcn obj{ws.obj, (int64_t)M * 3, 1, 3, DAL3_F32, a->pts.flags};
    // device sampler: the first min(count, M) object points are distinct, the rest are copies -> skipped by the head
    const int32_t* distinct = a->sampler == DAL3_SAMPLER_DEVICE ? a->counts : nullptr;
    // (the estimator's last FC layer and the decode of its output are one launch: fc39_decode_kernel)
    if (!a->two_stage) {
        // center = center_boxnet + init_box[:, :3] (static_model.py:132); yaw += init yaw (static_eval.py:280)
        const DecodeArgs d1{a->box_pred_one, a->init_box, 7, 0, nullptr, 0, a->init_box + 6, 7,
                            a->heading_residuals_one, a->size_residuals_one, a->center_one, a->boxes7};
        TRY(point_head_run(DAL3_HEAD_STATIC_BOX_EST, a->w_box_est_one, a->dtype, obj, B, M, a->box_pred_one, 39, ws.head, s,
                           distinct, &d1));
        return 0;
    }
    if (!a->w_box_est_two || !a->box_pred_two || !a->box_one || !a->center_one)
        return fail(DAL3_EINVAL, "static_forward: two_stage needs w_box_est_two, box_pred_two, box_one, center_one");
    // center_one += init_box[:, :3] in place (static_model.py:174); box_one (:176-190)
    const DecodeArgs d1{a->box_pred_one, a->init_box, 7, 1, nullptr, 0, a->init_box + 6, 7,
                        a->heading_residuals_one, a->size_residuals_one, a->center_one, a->box_one};
    TRY(point_head_run(DAL3_HEAD_STATIC_BOX_EST, a->w_box_est_one, a->dtype, obj, B, M, a->box_pred_one, 39, ws.head, s,
                       distinct, &d1));
    HIP_TRY(launch_recenter(ws.obj, B, M, a->init_box, a->box_one, a->bbox_gt, ws.obj2,
                            a->bbox_gt ? a->heading_class_label_two : nullptr,
                            a->bbox_gt ? a->heading_residuals_label_two : nullptr, s));
    const dal3_bcn obj2{ws.obj2, (int64_t)M * 3, 1, 3, DAL3_F32, a->pts.flags};
    // center_two += center_one (static_model.py:211); final yaw += box_one yaw (static_eval.py:282)
    const DecodeArgs d2{a->box_pred_two, a->center_one, 3, 1, nullptr, 0, a->box_one + 6, 7,
                        a->heading_residuals_two, a->size_residuals_two, a->center_two, a->boxes7};
    TRY(point_head_run(DAL3_HEAD_STATIC_BOX_EST, a->w_box_est_two, a->dtype, obj2, B, M, a->box_pred_two, 39, ws.head, s,
                       distinct, &d2));
    return 0;
}

// ---------------------------------------------------------------------------------- dynamic model
struct DynamicWs { InsSegWs seg; int32_t* pos; float* obj; HeadWs head; };
static DynamicWs carve_dynamic(Carver& c, int B, int N, int M) {
    DynamicWs w;
    w.seg = carve_ins_seg(c, B);
    w.pos = c.take<int32_t>((size_t)B * N);
    w.obj = c.take<float>((size_t)B * M * 4);
    w.head = carve_head(c, B);
    return w;
}
extern "C" size_t dal3_dynamic_workspace_bytes(int B, int N, int) {
    Carver c(nullptr, 0);
    carve_dynamic(c, B, N, 2560);
    return c.off;
}

extern "C" int dal3_dynamic_forward(const dal3_dynamic_args* a, int phases, dal3_stream stream) {
    if (!a) return fail(DAL3_EINVAL, "dynamic_forward: args is NULL");
    TRY(check_extent(a->B, a->N, "dynamic_forward"));
    TRY(check_extent(a->B, a->n_box, "dynamic_forward (n_box)"));
    if (!a->workspace) return fail(DAL3_EINVAL, "dynamic_forward: workspace is NULL");
    if (!(phases & DAL3_PHASE_ALL)) return fail(DAL3_EINVAL, "dynamic_forward: no phase selected");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = a->B, N = a->N, M = 2560;
    Carver c(a->workspace, a->workspace_bytes);
    const DynamicWs ws = carve_dynamic(c, B, N, M);
    if (!c.ok) return fail(DAL3_EWORKSPACE, "dynamic_forward: workspace needs %zu bytes, got %zu", c.off, a->workspace_bytes);

    if (phases & DAL3_PHASE_SEG) {
        TRY(ins_seg_run(a->w_ins_seg, a->dtype, 4, a->pts, B, N, a->logits, a->mask, nullptr, ws.seg, s));
        // (when the box phase follows in this call, its compaction kernel writes the same counts)
        if (a->counts && !(phases & DAL3_PHASE_BOX)) HIP_TRY(launch_segment_counts(a->mask, B, N, a->counts, s));
    }
    if (!(phases & DAL3_PHASE_BOX)) return 0;

    if (!a->embedding || !a->box_pred || !a->counts || !a->obj_idx || !a->w_point_emb || !a->w_box_emb || !a->w_box_est)
        return fail(DAL3_EINVAL, "dynamic_forward: null pointer in box phase");
    TRY(gather_run(a->mask, a->pts, B, N, 4, M, a->sampler, a->choice, a->seed, a->item_offset, a->counts, a->obj_idx,
                   ws.obj, ws.pos, s));
    const dal3_bcn obj{ws.obj, (int64_t)M * 4, 1, 4, DAL3_F32, a->pts.flags};
    // embedding = cat[point_e (256), box_e (128)] (dynamic_model.py:133-137): written side by side
    TRY(point_head_run(DAL3_HEAD_POINT_EMB, a->w_point_emb, a->dtype, obj, B, M, a->embedding, 384, ws.head, s,
                       a->sampler == DAL3_SAMPLER_DEVICE ? a->counts : nullptr));
    TRY(point_head_run(DAL3_HEAD_BOX_EMB, a->w_box_emb, a->dtype, a->box, B, a->n_box, a->embedding + 256, 384, ws.head, s));
    // forward() adds nothing to the centre; the eval driver adds init_box[:, :3] and yaw init_box[:, -2]
    const DecodeArgs dd{a->box_pred, nullptr, 0, 0, a->init_box8, 8, a->init_box8 ? a->init_box8 + 6 : nullptr, 8,
                        a->heading_residuals, a->size_residuals, nullptr, a->boxes7};
    TRY(fc_chain(view(a->w_box_est, fc_head_walk), a->embedding, 384, a->box_pred, 39, B,
                 ws.head.t1, ws.head.t2, s, &dd));
    return 0;
}

// ---------------------------------------------------------------------------------- CenterPoint's second stage
static bool map_dims_ok(int64_t B, int64_t H, int64_t W) { return B >= 0 && H >= 1 && W >= 1 && B <= 65535 && H <= 65535 && W <= 65535; }

extern "C" int dal3_bev_gather(const dal3_bev_gather_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "bev_gather: null args");
    const dal3_bev_gather_args& a = *args;
    if (!map_dims_ok(a.B, a.H, a.W) || a.C < 1 || a.C > 65535) return fail(DAL3_EINVAL, "bev_gather: bad B / H / W (<= 65535) / C (1 .. 65535)");
    if (a.n < 0 || a.n > DAL3_MAX_ITEMS) return fail(DAL3_EINVAL, "bev_gather: bad n (0 .. DAL3_MAX_ITEMS)");
    if (a.points_per_row < 1 || a.points_per_row > 5) return fail(DAL3_EINVAL, "bev_gather: points_per_row %d (1 .. 5)", (int)a.points_per_row);
    if (a.xy_stride < 2 || a.out_col_offset < 0 || a.out_row_stride < a.out_col_offset + (int64_t)a.points_per_row * a.C)
        return fail(DAL3_EINVAL, "bev_gather: xy_stride < 2, or the sections do not fit into a row of out_row_stride floats");
    if (!a.sample && (a.sample_index < 0 || (a.sample_index >= a.B && a.n > 0)))
        return fail(DAL3_EINVAL, "bev_gather: sample_index %d outside the %lld samples", (int)a.sample_index, (long long)a.B);
    if (a.n > 0 && (!a.map.data || !a.xy || !a.out)) return fail(DAL3_EINVAL, "bev_gather: null map / xy / out");
    if (!(a.voxel_size[0] > 0.f) || !(a.voxel_size[1] > 0.f) || !(a.out_stride > 0.f))
        return fail(DAL3_EINVAL, "bev_gather: voxel_size and out_stride must be positive");
    HIP_TRY(launch_bev_gather(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_box_points(const float* boxes, int64_t n, int cols, int num_point, float* out, dal3_stream stream) {
    if (n < 0 || n > DAL3_MAX_ITEMS || (cols != 7 && cols != 9) || (num_point != 1 && num_point != 5))
        return fail(DAL3_EINVAL, "box_points: bad n / cols (7 or 9) / num_point (1 or 5)");
    if (n > 0 && (!boxes || !out)) return fail(DAL3_EINVAL, "box_points: null boxes / out");
    HIP_TRY(launch_box_points(boxes, n, cols, num_point, out, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_roi_pack_floats(const dal3_roi_shape* shape) { return shape ? roi_pack_floats(shape) : 0; }

extern "C" int dal3_roi_pack(const dal3_roi_shape* shape, const dal3_layer* layers, int n_layers, const double* eps, float* out,
                             dal3_stream stream) {
    if (!shape || !layers || !out) return fail(DAL3_EINVAL, "roi_pack: null shape / layers / out");
    const int want = roi_layers(shape);
    if (want == 0)
        return fail(DAL3_EINVAL, "roi_pack: the shape is not served (1 .. 3 layers a list, widths multiples of 16 up to %d, "
                    "num_class 1, code_size 7 or 9)", DAL3_ROI_MAX_WIDTH);
    if (n_layers != want) return fail(DAL3_EINVAL, "roi_pack: %d layers given, the shape has %d", n_layers, want);
    for (int i = 0; i < n_layers; ++i) {
        const dal3_layer& L = layers[i];
        int c_in, c_out;
        roi_layer_dims(shape, i, &c_in, &c_out);
        if (L.c_in != c_in || L.c_out != c_out)
            return fail(DAL3_EINVAL, "roi_pack: layer %d is %d -> %d, the shape says %d -> %d", i, (int)L.c_in, (int)L.c_out, c_in, c_out);
        TRY(check_fold_layer("roi_pack", &L, i, eps ? eps[i] : 0.0, out));
    }
    HIP_TRY(launch_roi_pack(shape, layers, eps, out, static_cast<hipStream_t>(stream)));
    return 0;
}

static bool roi_dims_ok(int64_t B, int64_t M, int num_point, int C, int code_size) {
    return B >= 0 && M >= 0 && B <= 65535 && B * M <= (1 << 24) && (num_point == 1 || num_point == 5) && C >= 1 && C <= 65535 &&
           (code_size == 7 || code_size == 9);
}

extern "C" size_t dal3_roi_head_workspace_bytes(int64_t B, int64_t M, int num_point, int C, int code_size) {
    if (!roi_dims_ok(B, M, num_point, C, code_size)) return 0;
    return roi_head_workspace_bytes(B, M, num_point, C, code_size);
}

extern "C" int dal3_roi_head(const dal3_roi_head_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "roi_head: null args");
    const dal3_roi_head_args& a = *args;
    if (roi_layers(&a.shape) == 0) return fail(DAL3_EINVAL, "roi_head: the shape is not served (see dal3_roi_pack)");
    const int code = a.shape.code_size;
    if (!roi_dims_ok(a.B, a.M, a.num_point, a.C, code)) return fail(DAL3_EINVAL, "roi_head: bad B / M (B * M <= 2^24) / num_point (1 or 5) / C");
    if ((int64_t)a.num_point * a.C != a.shape.c_in)
        return fail(DAL3_EINVAL, "roi_head: num_point * C = %lld, the head takes %d inputs", (long long)a.num_point * a.C, (int)a.shape.c_in);
    if (!a.packed || (reinterpret_cast<uintptr_t>(a.packed) & 15)) return fail(DAL3_EINVAL, "roi_head: packed is null or not 16-byte aligned");
    const bool any = a.B > 0 && a.M > 0;
    if (a.keep) {
        if (a.T < 1 || a.T > DAL3_ROI_MAX_TASKS) return fail(DAL3_EINVAL, "roi_head: T %d (1 .. %d)", (int)a.T, DAL3_ROI_MAX_TASKS);
        if (a.box_cols != code) return fail(DAL3_EINVAL, "roi_head: boxes of %d columns for code_size %d", (int)a.box_cols, code);
        if (a.K < 0 || a.keep_stride < 0) return fail(DAL3_EINVAL, "roi_head: bad K / keep_stride");
        if (!map_dims_ok(a.B, a.H, a.W)) return fail(DAL3_EINVAL, "roi_head: bad H / W (1 .. 65535)");
        if (!(a.voxel_size[0] > 0.f) || !(a.voxel_size[1] > 0.f) || !(a.out_stride > 0.f))
            return fail(DAL3_EINVAL, "roi_head: voxel_size and out_stride must be positive");
        if (!a.keep_count || !a.seg_offsets || !a.status || (any && (!a.bev.data || (a.K > 0 && (!a.boxes || !a.scores || !a.labels)))))
            return fail(DAL3_EINVAL, "roi_head: null pointer in the fused form");
        if (any && (!a.workspace || (reinterpret_cast<uintptr_t>(a.workspace) & 7))) return fail(DAL3_EINVAL, "roi_head: workspace is null or misaligned");
    } else if (any && (!a.rois || !a.roi_scores || !a.roi_features)) {
        return fail(DAL3_EINVAL, "roi_head: the direct form needs rois, roi_scores and roi_features");
    }
    hipError_t e = hipSuccess;
    if (!launch_roi_head(args, static_cast<hipStream_t>(stream), &e))
        return fail(DAL3_EWORKSPACE, "roi_head: workspace of %zu bytes, %zu needed", a.workspace_bytes,
                    roi_head_workspace_bytes(a.B, a.M, a.num_point, a.C, code));
    HIP_TRY(e);
    return 0;
}

extern "C" int dal3_roi_post(const float* box_preds, const float* cls_preds, const float* roi_scores, int64_t n, int code_size,
                             float* out_boxes, float* out_scores, dal3_stream stream) {
    if (n < 0 || n > (1 << 24) || (code_size != 7 && code_size != 9)) return fail(DAL3_EINVAL, "roi_post: bad n / code_size (7 or 9)");
    if (n > 0 && (!box_preds || !cls_preds || !roi_scores)) return fail(DAL3_EINVAL, "roi_post: null input");
    HIP_TRY(launch_roi_post(box_preds, cls_preds, roi_scores, n, code_size, out_boxes, out_scores, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_roi_targets(const dal3_roi_targets_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "roi_targets: null args");
    const dal3_roi_targets_args& a = *args;
    if (a.B < 0 || a.B > 65535 || a.M < 1 || a.M > DAL3_ROI_TRAIN_MAX_M || a.R < 1 || a.R > DAL3_ROI_TRAIN_MAX_R || a.G < 1 ||
        a.G > DAL3_ROI_TRAIN_MAX_G || (a.code_size != 7 && a.code_size != 9))
        return fail(DAL3_EINVAL, "roi_targets: bad B / M (1 .. %d) / R (1 .. %d) / G (1 .. %d) / code_size (7 or 9)",
                    DAL3_ROI_TRAIN_MAX_M, DAL3_ROI_TRAIN_MAX_R, DAL3_ROI_TRAIN_MAX_G);
    if (a.cls_score_type != DAL3_ROI_CLS_SCORE_ROI_IOU && a.cls_score_type != DAL3_ROI_CLS_SCORE_CLS)
        return fail(DAL3_EINVAL, "roi_targets: cls_score_type %d", (int)a.cls_score_type);
    if (a.fg_per_image < 0 || !(a.hard_bg_ratio >= 0.0 && a.hard_bg_ratio <= 1.0) || !(a.cls_thresh_span > 0.f))
        return fail(DAL3_EINVAL, "roi_targets: bad fg_per_image / hard_bg_ratio (0 .. 1) / cls_thresh_span (> 0)");
    if (a.B == 0) return 0;
    if (a.keep) {
        if (a.T < 1 || a.T > DAL3_ROI_MAX_TASKS) return fail(DAL3_EINVAL, "roi_targets: T %d (1 .. %d)", (int)a.T, DAL3_ROI_MAX_TASKS);
        if (a.K < 0 || a.keep_stride < 0) return fail(DAL3_EINVAL, "roi_targets: bad K / keep_stride");
        if (!a.boxes || !a.scores || !a.labels || !a.keep_count || !a.seg_offsets)
            return fail(DAL3_EINVAL, "roi_targets: null pointer in the fused form");
    } else if (!a.rois || !a.roi_scores || !a.roi_labels) {
        return fail(DAL3_EINVAL, "roi_targets: the direct form needs rois, roi_scores and roi_labels");
    }
    if (!a.gt || !a.draws || !a.slot || !a.sample || !a.out_rois || !a.out_labels || !a.out_scores || !a.gt_iou || !a.gt_src ||
        !a.reg_valid || !a.cls_labels || !a.gt_of_rois || !a.out_boxes || !a.status)
        return fail(DAL3_EINVAL, "roi_targets: null gt / draws / output / status");
    HIP_TRY(launch_roi_targets(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_roi_loss(const float* rcnn_cls, const float* rcnn_reg, int64_t N, int code_size, const float* cls_labels,
                             const int32_t* reg_valid, const float* gt_of_rois, const float* code_weights, float cls_weight,
                             float reg_weight, float* loss, float* d_cls, float* d_reg, dal3_stream stream) {
    if (N < 0 || N > (1 << 24) || (code_size != 7 && code_size != 9)) return fail(DAL3_EINVAL, "roi_loss: bad N / code_size (7 or 9)");
    if (!rcnn_cls || !rcnn_reg || !cls_labels || !reg_valid || !gt_of_rois || !code_weights || !loss || !d_cls || !d_reg)
        return fail(DAL3_EINVAL, "roi_loss: null argument");
    HIP_TRY(launch_roi_loss(rcnn_cls, rcnn_reg, N, code_size, cls_labels, reg_valid, gt_of_rois, code_weights, cls_weight, reg_weight,
                            loss, d_cls, d_reg, static_cast<hipStream_t>(stream)));
    return 0;
}


extern "C" int dal3_center_targets(const dal3_center_targets_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "center_targets: null args");
    const dal3_center_targets_args& a = *args;
    if (!map_dims_ok(a.B, a.H, a.W) || a.G < 1 || a.G > (1 << 20)) return fail(DAL3_EINVAL, "center_targets: bad B / G (1 .. 2^20) / H / W (1 .. 65535)");
    if (a.T < 1 || a.T > DAL3_ROI_MAX_TASKS) return fail(DAL3_EINVAL, "center_targets: T %d (1 .. %d)", (int)a.T, DAL3_ROI_MAX_TASKS);
    if (a.max_objs < 1 || a.max_objs > DAL3_CENTER_MAX_OBJS) return fail(DAL3_EINVAL, "center_targets: max_objs %d (1 .. %d)", (int)a.max_objs, DAL3_CENTER_MAX_OBJS);
    if (!(a.voxel_size[0] > 0.f) || !(a.voxel_size[1] > 0.f) || !(a.out_size_factor > 0.f))
        return fail(DAL3_EINVAL, "center_targets: voxel_size and out_size_factor must be positive");
    if (!(a.gaussian_overlap >= 0.0 && a.gaussian_overlap < 1.0) || a.min_radius < 0 || a.min_radius > 65535)
        return fail(DAL3_EINVAL, "center_targets: bad gaussian_overlap (0 <= . < 1) / min_radius (0 .. 65535)");
    for (int t = 0; t < a.T; ++t) {
        if (a.num_class[t] < 1 || a.num_class[t] > DAL3_CENTER_MAX_CLASSES)
            return fail(DAL3_EINVAL, "center_targets: task %d has %d classes (1 .. %d)", t, (int)a.num_class[t], DAL3_CENTER_MAX_CLASSES);
        if (a.num_class[t] * a.H * a.W >= ((int64_t)1 << 31)) return fail(DAL3_EINVAL, "center_targets: task %d's map has 2^31 elements or more", t);
        if (!a.hm[t] || !a.anno_box[t] || !a.ind[t] || !a.mask[t] || !a.cat[t]) return fail(DAL3_EINVAL, "center_targets: null output of task %d", t);
    }
    if (!a.gt || !a.status) return fail(DAL3_EINVAL, "center_targets: null gt / status");
    HIP_TRY(launch_center_targets(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_center_loss_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
    if (!map_dims_ok(B, H, W) || C < 1 || C > DAL3_CENTER_MAX_CLASSES) return 0;
    return center_loss_workspace_bytes(B, C, H, W);
}

extern "C" int dal3_center_loss(const dal3_center_loss_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "center_loss: null args");
    const dal3_center_loss_args& a = *args;
    if (!map_dims_ok(a.B, a.H, a.W) || a.C < 1 || a.C > DAL3_CENTER_MAX_CLASSES) return fail(DAL3_EINVAL, "center_loss: bad B / H / W (1 .. 65535) / C (1 .. %d)", DAL3_CENTER_MAX_CLASSES);
    if (a.n_cols != 8 && a.n_cols != 10) return fail(DAL3_EINVAL, "center_loss: n_cols %d (8 or 10)", (int)a.n_cols);
    if (a.max_objs < 1 || a.max_objs > DAL3_CENTER_MAX_OBJS) return fail(DAL3_EINVAL, "center_loss: max_objs %d (1 .. %d)", (int)a.max_objs, DAL3_CENTER_MAX_OBJS);
    if (a.B * (a.C + a.n_cols) * a.H * a.W >= ((int64_t)1 << 31)) return fail(DAL3_EINVAL, "center_loss: B * (C + n_cols) * H * W must stay below 2^31");
    if ((a.vel.data != nullptr) != (a.n_cols == 10)) return fail(DAL3_EINVAL, "center_loss: the vel map goes with n_cols 10, and only with it");
    if (!a.out) return fail(DAL3_EINVAL, "center_loss: null out");
    if (a.B == 0) return fail(DAL3_EINVAL, "center_loss: an empty batch has no loss");
    if (!a.hm.data || !a.reg.data || !a.height.data || !a.dim.data || !a.rot.data || !a.target_hm || !a.anno_box || !a.ind || !a.mask ||
        !a.cat || !a.grad)
        return fail(DAL3_EINVAL, "center_loss: null map / target / grad");
    if (!a.workspace || (reinterpret_cast<uintptr_t>(a.workspace) & 7)) return fail(DAL3_EINVAL, "center_loss: workspace is null or misaligned");
    hipError_t e = hipSuccess;
    if (!launch_center_loss(args, static_cast<hipStream_t>(stream), &e))
        return fail(DAL3_EWORKSPACE, "center_loss: workspace of %zu bytes, %zu needed", a.workspace_bytes,
                    center_loss_workspace_bytes(a.B, a.C, a.H, a.W));
    HIP_TRY(e);
    return 0;
}

// ---------------------------------------------------------------------------------- the training input
static bool aug_dims_ok(int64_t B, int32_t max_gt, int64_t max_cand) {
    return B >= 0 && B <= 65535 && max_gt >= 1 && max_gt <= DAL3_AUG_MAX_BOXES && max_cand >= 1 && max_cand <= DAL3_AUG_MAX_CAND;
}

extern "C" int dal3_gt_paste_select(const dal3_gt_paste_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "gt_paste_select: null args");
    const dal3_gt_paste_args& a = *args;
    if (!aug_dims_ok(a.B, a.max_gt, a.max_cand))
        return fail(DAL3_EINVAL, "gt_paste_select: bad B (<= 65535) / max_gt (1 .. %d) / max_cand (1 .. %d)", DAL3_AUG_MAX_BOXES, DAL3_AUG_MAX_CAND);
    if (!a.gt_boxes || !a.gt_classes || !a.gt_counts || !a.cand_boxes || !a.cand_group || !a.cand_counts || !a.accept || !a.status)
        return fail(DAL3_EINVAL, "gt_paste_select: null argument");
    HIP_TRY(launch_gt_paste_select(args, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" size_t dal3_augment_points_workspace_bytes(int64_t B, int64_t n) {
    if (B < 0 || B > 65535 || n < 0 || n >= ((int64_t)1 << 31)) return 0;
    return augment_points_workspace_bytes(B, n);
}

extern "C" int dal3_augment_points(const dal3_augment_points_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "augment_points: null args");
    const dal3_augment_points_args& a = *args;
    if (a.B < 0 || a.B > 65535 || a.n < 0 || a.n >= ((int64_t)1 << 31) || a.n_scene < 0 || a.db_rows < 0)
        return fail(DAL3_EINVAL, "augment_points: bad B (<= 65535) / n (< 2^31) / n_scene / db_rows");
    if (a.F < 3 || a.F > 8) return fail(DAL3_EINVAL, "augment_points: F %d (3 .. 8)", (int)a.F);
    if (a.max_cand < 1 || a.max_cand > DAL3_AUG_MAX_CAND || a.max_workgroups < 0)
        return fail(DAL3_EINVAL, "augment_points: bad max_cand (1 .. %d) / max_workgroups", DAL3_AUG_MAX_CAND);
    if (!a.status || !a.workspace || (reinterpret_cast<uintptr_t>(a.workspace) & 7)) return fail(DAL3_EINVAL, "augment_points: null status, or workspace null or misaligned");
    if (a.n > 0 && a.B > 0) {
        if (!a.out || !a.out_offsets || !a.scene_offsets || !a.cand_counts || !a.cand_seg_start || !a.cand_rows || !a.cand_db_row ||
            (a.n_scene > 0 && !a.scene) || (a.db_rows > 0 && (!a.db_points || !a.cand_boxes || !a.accept)) || (a.transform && !a.xform))
            return fail(DAL3_EINVAL, "augment_points: null argument");
        if (a.F == 4 && ((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.scene) | reinterpret_cast<uintptr_t>(a.db_points)) & 15))
            return fail(DAL3_EINVAL, "augment_points: four-column rows must be 16-byte aligned");
    }
    hipError_t e = hipSuccess;
    if (!launch_augment_points(args, static_cast<hipStream_t>(stream), &e))
        return fail(DAL3_EWORKSPACE, "augment_points: workspace of %zu bytes, %zu needed", a.workspace_bytes, augment_points_workspace_bytes(a.B, a.n));
    HIP_TRY(e);
    return 0;
}

extern "C" int dal3_augment_boxes(const dal3_augment_boxes_args* args, dal3_stream stream) {
    if (!args) return fail(DAL3_EINVAL, "augment_boxes: null args");
    const dal3_augment_boxes_args& a = *args;
    if (!aug_dims_ok(a.B, a.max_gt, a.max_cand))
        return fail(DAL3_EINVAL, "augment_boxes: bad B (<= 65535) / max_gt (1 .. %d) / max_cand (1 .. %d)", DAL3_AUG_MAX_BOXES, DAL3_AUG_MAX_CAND);
    if (a.max_objs < 1 || a.max_objs > DAL3_CENTER_MAX_OBJS || a.n_classes < 1 || a.n_classes > DAL3_CENTER_MAX_CLASSES)
        return fail(DAL3_EINVAL, "augment_boxes: bad max_objs (1 .. %d) / n_classes (1 .. %d)", DAL3_CENTER_MAX_OBJS, DAL3_CENTER_MAX_CLASSES);
    if (!a.gt_boxes || !a.gt_classes || !a.gt_counts || !a.out || !a.out_count || !a.status || (a.transform && !a.xform) ||
        (a.accept && (!a.cand_boxes || !a.cand_classes || !a.cand_counts)))
        return fail(DAL3_EINVAL, "augment_boxes: null argument");
    HIP_TRY(launch_augment_boxes(args, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---------------------------------------------------------------------------------- the optimiser step
static bool optim_flat_ok(int64_t n_flat) { return n_flat > 0 && (n_flat & 3) == 0 && n_flat < ((int64_t)1 << 40); }
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int64_t dal3_optim_partials(int64_t n_flat) { return optim_flat_ok(n_flat) ? optim_partials(n_flat) : 0; }

extern "C" int dal3_optim_grad_norm(const float* grad, int64_t n_flat, dal3_optim_hyper* hyper, double* partials, dal3_stream stream) {
    if (!optim_flat_ok(n_flat)) return fail(DAL3_EINVAL, "optim_grad_norm: n_flat must be a positive multiple of 4 below 2^40");
    if (!grad || !hyper || !partials || !aligned16(grad) || !aligned16(hyper)) return fail(DAL3_EINVAL, "optim_grad_norm: null or misaligned argument");
    HIP_TRY(launch_optim_grad_norm(grad, n_flat, hyper, partials, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_optim_step(const dal3_optim_chunk* chunks, int64_t n_chunks, float* grad, float* exp_avg, float* exp_avg_sq,
                               int64_t n_flat, const double* partials, dal3_optim_hyper* hyper, dal3_stream stream) {
    if (!optim_flat_ok(n_flat)) return fail(DAL3_EINVAL, "optim_step: n_flat must be a positive multiple of 4 below 2^40");
    if (n_chunks < 1 || n_chunks > 0x7fffffff) return fail(DAL3_EINVAL, "optim_step: bad n_chunks");
    if (!chunks || !grad || !exp_avg || !exp_avg_sq || !partials || !hyper || !aligned16(grad) || !aligned16(exp_avg) ||
        !aligned16(exp_avg_sq) || !aligned16(hyper))
        return fail(DAL3_EINVAL, "optim_step: null or misaligned argument");
    HIP_TRY(launch_optim_step(chunks, n_chunks, grad, exp_avg, exp_avg_sq, n_flat, partials, hyper, static_cast<hipStream_t>(stream)));
    return 0;
}

extern "C" int dal3_optim_total_norm(const double* partials, int64_t n_partials, float* out, dal3_stream stream) {
    if (!partials || !out || n_partials < 1) return fail(DAL3_EINVAL, "optim_total_norm: null argument or no partials");
    HIP_TRY(launch_optim_total_norm(partials, n_partials, out, static_cast<hipStream_t>(stream)));
    return 0;
}
