// k_pred.h -- FilterSpec on an already loaded scalar: the one place that says what
// `(field OP ref) != negate` means for integer and float columns
// (getComparisonFuncForComparisonType, filter.go:236-263).  Device code and plain host C++17
// (the sanitizer driver runs it on the CPU).
#pragma once

#include <cstdint>

#include "../../include/igx.h"

#ifdef __HIPCC__
#define IGX_HD __host__ __device__
#else
#define IGX_HD
#endif

// sign-extend the low `width` (1, 2, 4 or 8) bytes of v
IGX_HD inline __attribute__((always_inline)) uint64_t sext(uint64_t v, uint32_t width) {
    const uint32_t sh = 64u - 8u * width;
    return sh ? (uint64_t)(((int64_t)(v << sh)) >> sh) : v;
}

// three-way compare of a zero-extended value of `width` bytes against a zero-extended
// reference: -1, 0, 1, or 2 for unordered (a NaN on either side)
IGX_HD inline __attribute__((always_inline)) int pred_cmp3(uint64_t v, uint64_t ref, uint32_t width, uint32_t kind) {
    if (kind == IGX_KIND_FLOAT) {
        double x, y;
        if (width == 4) {
            x = __builtin_bit_cast(float, (uint32_t)v);
            y = __builtin_bit_cast(float, (uint32_t)ref);
        } else {
            x = __builtin_bit_cast(double, v);
            y = __builtin_bit_cast(double, ref);
        }
        return (x != x || y != y) ? 2 : (x < y ? -1 : (x > y ? 1 : 0));
    }
    if (kind == IGX_KIND_INT) {
        const int64_t x = (int64_t)sext(v, width), y = (int64_t)sext(ref, width);
        return x < y ? -1 : (x > y ? 1 : 0);
    }
    return v < ref ? -1 : (v > ref ? 1 : 0);
}

// the operator table: unordered and an unknown cmp are false before the XOR with negate
IGX_HD inline __attribute__((always_inline)) bool pred_op(int c, uint32_t cmp, uint32_t neg) {
    const bool r = c != 2 && ((cmp == IGX_CMP_EQ && c == 0) || (cmp == IGX_CMP_LT && c < 0) ||
                              (cmp == IGX_CMP_LE && c <= 0) || (cmp == IGX_CMP_GT && c > 0) ||
                              (cmp == IGX_CMP_GE && c >= 0));
    return r != (neg != 0);
}

IGX_HD inline __attribute__((always_inline)) bool pred_scalar(uint64_t v, uint64_t ref, uint32_t width, uint32_t kind,
                                                              uint32_t cmp, uint32_t neg, uint32_t cnt) {
    if (cmp == IGX_CMP_IN) {   // set membership: cnt values of `width` bytes packed in ref
        const uint64_t m = width >= 8 ? ~0ull : ((1ull << (8 * width)) - 1);
        bool in = false;
        for (uint32_t i = 0; i < cnt; ++i) in = in || v == ((ref >> (8 * width * i)) & m);
        return in != (neg != 0);
    }
    return pred_op(pred_cmp3(v, ref, width, kind), cmp, neg);
}
