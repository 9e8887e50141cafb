// The order contract's key, the list words built on it and the wave helpers of the search family (gfx950): ONE definition for
// topk.hip, topk_wide.hip, rank.hip, search.hip, search_filter.hip, search_compact.hip and search_compact_filter.hip.
//
// Order contract: larger value first, the lower column first among equal values (-0 == +0), NaN above every number, the lower column
// first among NaNs, -inf / -1 behind the last entry.  On keys and words that is plain unsigned order.
#pragma once
#include "sc_common.h"

constexpr uint32_t TK_EMPTY = 0u;            // below every real key (-inf maps to 0x007fffff): no column has key 0
constexpr uint32_t TK_NAN = 0xffffffffu;     // above +inf (0xff800000)

// fp32 -> uint32 with the order of the contract: a < b as floats <=> key(a) < key(b); -0 and +0 share a key; every NaN is TK_NAN
__device__ __forceinline__ uint32_t tk_key(float v) {
    const uint32_t u = __float_as_uint(v);
    uint32_t k = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
    if ((u & 0x7fffffffu) > 0x7f800000u) k = TK_NAN;
    if (k == 0x7fffffffu) k = 0x80000000u;
    return k;
}
// the key mapped back: a zero comes back as +0, every NaN as the default NaN, TK_EMPTY as -inf
__device__ __forceinline__ float tk_value(uint32_t k) {
    if (k == TK_EMPTY) return -INFINITY;
    if (k == TK_NAN) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// the float a group of scores is tested against: the value of a list's last key, NaN when the list is not full or its tail is a NaN
// (every group then takes the exact path)
__device__ __forceinline__ float tk_threshold(uint32_t k) {
    if (k == TK_EMPTY || k == TK_NAN) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// A list entry: key << 32 | ~column.  Words of distinct columns are distinct, so the order is total, and ~column puts the lower
// column first among equal keys.  0 = no entry: it decodes to -inf / -1.
__device__ __forceinline__ uint64_t tk_word(uint32_t key, int col) { return ((uint64_t)key << 32) | (uint32_t)~(uint32_t)col; }
__device__ __forceinline__ uint32_t tk_word_key(uint64_t w) { return (uint32_t)(w >> 32); }
__device__ __forceinline__ int tk_word_col(uint64_t w) { return (int)~(uint32_t)w; }

// lane i <- lane i - 1 over the whole wave (DPP wave_shr:1, an ALU move: no LDS round trip); lane 0 gets 0 and is handled by the caller
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

// 64-lane maximum of a 64-bit word, the same value in every lane
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t best) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o);
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, o);
        const uint64_t q = ((uint64_t)hi << 32) | lo;
        best = q > best ? q : best;
    }
    return best;
}

// 16 bytes per lane from global memory straight into LDS (the wave's 64 chunks land contiguously behind lds_wave_base)
__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
