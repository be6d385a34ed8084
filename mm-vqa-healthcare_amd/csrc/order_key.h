// The 64-bit order key of the search and evaluation kernels: (monotone image of an fp32 value) << 32 | (2^32 - 1 - index).  The
// maximum of a set of keys is the greatest value and, among equal values, the lowest index; keys of distinct indices are distinct,
// so a maximum over them is the same whatever the order of the fold.  No key is 0: 0 stands for "no key".
// csrc/beam.hip builds its keys with make_key from scores that hold no NaN; every other kernel builds them with eval_key, whose
// rule is torch.argmax's, and reads them back with key_index / key_value.
#pragma once
#include "common.h"

namespace {

DEVINL uint32_t ord32(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEVINL float unord32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
DEVINL uint64_t make_key(float score, uint32_t flat) { return ((uint64_t)ord32(score) << 32) | (uint64_t)(0xffffffffu - flat); }

// u = the bits of an fp32 value.  -0 is folded onto +0, and every NaN of either sign takes the top image 2^32 - 1: a NaN beats
// every number and the first NaN wins.  bf16 widens to fp32 exactly (16 zero bits), so the compare is the same compare.
DEVINL uint64_t eval_key(uint32_t u, uint32_t col) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return ((uint64_t)0xffffffffu << 32) | (uint64_t)(0xffffffffu - col);   // NaN: above +inf
    return make_key(__uint_as_float(u == 0x80000000u ? 0u : u), col);                                           // -0 -> +0
}
DEVINL uint32_t bits_of(float v) { return __float_as_uint(v); }
DEVINL uint32_t bits_of(bf16_t v) { return (uint32_t)v << 16; }

DEVINL uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }
DEVINL int64_t key_index(uint64_t g) { return (int64_t)(0xffffffffu - (uint32_t)g); }
// ... or -1 for "no key" and for an index outside [0, n): what is returned is never an address then
DEVINL int64_t key_index_in(uint64_t g, int64_t n) {
    const int64_t i = key_index(g);
    return (g == 0 || i >= n) ? -1 : i;
}
// the value behind an eval_key: exact but for -0 -> +0 and the NaN payload
DEVINL float key_value(uint64_t g) {
    const uint32_t hi = (uint32_t)(g >> 32);
    return hi == 0xffffffffu ? __uint_as_float(0x7fc00000u) : unord32(hi);
}

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
