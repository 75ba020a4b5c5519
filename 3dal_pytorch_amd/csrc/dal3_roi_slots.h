// dal3_roi_slots.h -- what dal3_roi.hip (the eval route) and dal3_roi_train.hip (the training route) share, so that a slot
// is the same row on both: the slot resolution of dal3_roi_head's step (a).
#pragma once
#include <stdint.h>

namespace {

// Step (a) for slot m of sample b: walks the sample's tasks over keep_count (T <= 16 segments: a walk, not a scan).
// before: the sample's kept rows over every task; row: the slot's row of boxes / scores / labels (-1: the slot lies past
// the count, -2: found and unusable); task: the row's task; bad: a keep_count beyond keep_stride or a row outside [0, K).
__device__ __forceinline__ void roi_slot_row(const int32_t* keep, const int32_t* keep_count, const int64_t* seg_offsets, int T, int B,
                                             int64_t K, int64_t keep_stride, int b, int m, int64_t& before, int64_t& row, int& task,
                                             int& bad) {
    before = 0, row = -1, task = 0, bad = 0;
    for (int t = 0; t < T; ++t) {
        const int64_t f = (int64_t)t * B + b;
        int64_t c = keep_count[f];
        if (c < 0 || c > keep_stride) {
            bad = 1;
            c = c < 0 ? 0 : keep_stride;
        }
        if (row < 0 && m < before + c) {
            row = seg_offsets[f] + keep[f * keep_stride + (m - before)];
            task = t;
            if (row < 0 || row >= K) {
                bad = 1;
                row = -2;                // found, unusable: the slot is empty
            }
        }
        before += c;
    }
}

}  // namespace
