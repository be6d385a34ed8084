// The 64-bit order key of the search kernels (csrc/beam.hip, csrc/greedy.hip): (monotone image of an fp32 value) << 32 |
// (2^32 - 1 - index).  The maximum of a set of keys is the greatest value and, among equal values, the lowest index; keys of distinct
// indices are distinct, so a maximum over them is the same whatever the order of the fold.
#pragma once
#include "common.h"

namespace {

DEVINL uint32_t ord32(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEVINL float unord32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
DEVINL uint64_t make_key(float score, uint32_t flat) { return ((uint64_t)ord32(score) << 32) | (uint64_t)(0xffffffffu - flat); }

DEVINL uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

}  // namespace
