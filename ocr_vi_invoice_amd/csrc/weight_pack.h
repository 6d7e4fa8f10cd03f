// Host: the steps every f16x2 weight packer shares -- the per-layer scale, the hi / lo split, the (hi, lo) quartet form and the row of
// an LDS image.  What differs between the packers (pack_conv, pack_bneck_tail, pack_mlp_x2_stream, pack_lin_x2_stream) is only their
// gather: which weight lands in which k-slot of which row.  The swizzles a row is stored under are common.h's swz128 / swz_halo, the
// functions the kernels read with.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"

namespace ocrvi {

// One power of two per layer that puts the largest |w| into [2^13, 2^14): far from fp16's 65504, and every weight within 2^-17 of the
// largest keeps a NORMAL lo half (full 2^-23 relative accuracy; smaller ones are off by at most 2^-39 of the largest).  The kernels'
// epilogues multiply the accumulator by the inverse, which is exact.  1 for an all-zero or non-finite tensor.
static inline float f16x2_weight_scale(const float* w, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, fabsf(w[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.f;
    int e = 0;
    (void)frexpf(mx, &e);                       // mx in [2^(e-1), 2^e)
    return ldexpf(1.0f, std::min(std::max(14 - e, -100), 100));
}

// x = hi + lo, hi = RN16(x), lo = RN16(x - hi) (common.h, f16x2_t)
static inline void f16x2_split(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// (hi, lo) quartet form, for kernels that read a lane's 8 k-slots as two 16-byte operands without regrouping them in registers: a 32-byte
// group of 8 consecutive k-slots in chunk form, four 8-byte pieces [hi4 lo4 | hi4' lo4'], becomes [hi4 hi4' | lo4 lo4']
static inline void f16x2_quartets(char* group) { std::swap_ranges(group + 8, group + 16, group + 16); }

// One 128-byte row of an LDS image: v = 32 fp32 values in the consumer's k-slot order; 16-byte position 2 q holds the hi halves of
// k-slots 8 q .. 8 q + 7, position 2 q + 1 their lo halves (of v * scale), and position P is stored at P ^ sw.
static inline void f16x2_put_row(const float* v, float scale, int sw, char* dst) {
    _Float16 halves[64];
    char* row = (char*)halves;
    convert_to_dtype(v, 32, OCRVI_F16X2, halves, scale);
    for (int q = 0; q < 4; ++q) f16x2_quartets(row + 32 * q);
    for (int P = 0; P < 8; ++P) memcpy(dst + ((P ^ sw) << 4), row + 16 * P, 16);
}

}  // namespace ocrvi
