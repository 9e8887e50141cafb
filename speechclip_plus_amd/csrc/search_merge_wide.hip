// Wide merge of per-shard search lists (gfx950): S best-first lists of up to 1024 entries per query, one per disjoint row range of a
// gallery, become one list under the order contract of search_common.h.  The piece behind retrieval.search_sharded: every shard is
// searched by retrieval.search on its own (any k the wide selection serves), this file only merges.
//   sc_search_merge_lists_f32   part_vals / part_idx: entry (s, q, j) at s * shard_stride + q * k + j (fp32 / int32 row OF THE SHARD, -1 =
//                               no entry), row0 [S] int64 = the global row of every shard's row 0
//                               -> vals [nQ, k] fp32, idx [nQ, k] int32 global row, best first
//
// The order is topk.hip's contract over GLOBAL rows: larger value first, the lower global row first among equal values (-0 == +0), NaN
// above every number, the lower global row first among NaNs, -inf / -1 behind the last entry.  An input entry is a filler iff its
// part_idx < 0, whatever its value; a real -inf with part_idx >= 0 is an entry and ranks ahead of every filler.  The sort key of an
// entry is tk_word(tk_key(value), row0[s] + part_idx) - no real entry has the word 0, so 0 means "no entry" - and the value's own 32
// bits travel beside the word as a payload: -0 stays -0 and a NaN keeps its payload, which sc_search_merge_u64 (it decodes the key)
// cannot do.  Words of distinct global rows are distinct, so the order is total and the result does not depend on S.
//
// One 256-thread workgroup per group of queries; a query owns kp = k rounded up to a power of two consecutive slots of one LDS array
// of 1024 words + 1024 payloads (12 KiB).  kp >= 256: one query per workgroup, kp / 256 slots per thread; kp < 256: 256 / kp queries
// per workgroup, one slot per thread.
//   1. shard 0's list is loaded as it lies (slots k .. kp - 1: no entry).
//   2. every further shard: slot i takes the larger of its word and the word of the shard's entry kp - 1 - i (the list REVERSED, read
//      straight from global memory).  Both lists are best first, so that leaves the kp largest words of the union as a bitonic
//      sequence; log2(kp) compare-exchange steps (strides kp / 2 .. 1, a barrier in front of each) sort it again, descending.
//   3. store: idx = the word's row (~low half), vals = the payload; -inf / -1 where the word is 0.
// The kernel relies on the lists being best first for its RESULT only: no address is computed from a value, a row or a word, every
// global access is indexed by s < S, q < nQ, j < k alone.  No atomics, nothing allocated, no runtime-indexed register arrays.
#include "search_common.h"

namespace {

constexpr int ML_THREADS = 256;
constexpr int ML_KMAX = 1024;

struct MergeShared {
    uint64_t word[ML_KMAX];
    uint32_t bits[ML_KMAX];                  // the value's own 32 bits, moved with its word
};

__global__ __launch_bounds__(ML_THREADS) void search_merge_lists_kernel(const uint32_t* __restrict__ part_vals,
                                                                        const int32_t* __restrict__ part_idx, int64_t shard_stride,
                                                                        const int64_t* __restrict__ row0, int nQ, int S, int k, int lg,
                                                                        float* __restrict__ vals, int32_t* __restrict__ idx) {
    __shared__ MergeShared s;
    const int tid = threadIdx.x;
    const int kp = 1 << lg;                                  // slots per query
    const int G = kp >= ML_THREADS ? 1 : ML_THREADS >> lg;   // queries per workgroup
    const int slots = G << lg;                               // 256 below kp = 256, kp above
    const int64_t q0 = (int64_t)blockIdx.x * G;

    // ---- 1. + 2. shard by shard
    for (int sh = 0; sh < S; ++sh) {
        const int64_t base = sh * shard_stride;
        const int64_t first = row0[sh];
        if (sh > 0) __syncthreads();                         // the last compare-exchange step of the shard before
        for (int e = tid; e < slots; e += ML_THREADS) {
            const int i = e & (kp - 1);
            const int64_t q = q0 + (e >> lg);
            const int j = sh == 0 ? i : kp - 1 - i;
            uint64_t w = 0ull;
            uint32_t b = 0xff800000u;                        // -inf
            if (q < nQ && j < k) {
                const int64_t o = base + q * k + j;
                const int32_t c = part_idx[o];
                if (c >= 0) {
                    b = part_vals[o];
                    w = tk_word(tk_key(__uint_as_float(b)), (int)(first + c));
                }
            }
            if (sh == 0 || w > s.word[e]) {
                s.word[e] = w;
                s.bits[e] = b;
            }
        }
        if (sh == 0) continue;
        for (int stride = kp >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int p = tid; p < (slots >> 1); p += ML_THREADS) {
                const int i = p & ((kp >> 1) - 1);
                const int lo = ((p >> (lg - 1)) << lg) + 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const uint64_t x = s.word[lo], y = s.word[hi];
                if (x < y) {
                    const uint32_t bx = s.bits[lo], by = s.bits[hi];
                    s.word[lo] = y;
                    s.word[hi] = x;
                    s.bits[lo] = by;
                    s.bits[hi] = bx;
                }
            }
        }
    }
    __syncthreads();

    // ---- 3. store
    for (int e = tid; e < slots; e += ML_THREADS) {
        const int i = e & (kp - 1);
        const int64_t q = q0 + (e >> lg);
        if (q < nQ && i < k) {
            const uint64_t w = s.word[e];
            const int64_t o = q * k + i;
            vals[o] = w ? __uint_as_float(s.bits[e]) : -INFINITY;
            idx[o] = w ? tk_word_col(w) : -1;
        }
    }
}

}  // namespace

extern "C" int sc_search_merge_lists_f32(const float* part_vals, const int32_t* part_idx, int64_t shard_stride, const int64_t* row0,
                                         int32_t nQ, int32_t S, int32_t k, float* vals, int32_t* idx, void* stream) {
    SC_CHECK(nQ >= 0, "sc_search_merge_lists_f32: nQ >= 0 (nQ %d)", nQ);
    SC_CHECK(k >= 1 && k <= ML_KMAX, "sc_search_merge_lists_f32: 1 <= k <= 1024 (k %d)", k);
    SC_CHECK(S >= 1, "sc_search_merge_lists_f32: S >= 1 (S %d)", S);
    SC_CHECK(shard_stride >= 0, "sc_search_merge_lists_f32: shard_stride >= 0 (shard_stride %lld)", (long long)shard_stride);
    if (nQ == 0) return 0;
    SC_CHECK(S == 1 || shard_stride >= (int64_t)nQ * k, "sc_search_merge_lists_f32: shard_stride >= nQ k (shard_stride %lld, nQ %d, k %d)",
             (long long)shard_stride, nQ, k);
    SC_CHECK(part_vals && part_idx && row0 && vals && idx, "sc_search_merge_lists_f32: null pointer");
    SC_CHECK(((uintptr_t)part_vals % 4) == 0 && ((uintptr_t)part_idx % 4) == 0 && ((uintptr_t)vals % 4) == 0 && ((uintptr_t)idx % 4) == 0,
             "sc_search_merge_lists_f32: part_vals, part_idx, vals and idx must be 4-byte aligned");
    SC_CHECK(((uintptr_t)row0 % 8) == 0, "sc_search_merge_lists_f32: row0 must be 8-byte aligned");
    int lg = 0;
    while ((1 << lg) < k) ++lg;
    const int G = (1 << lg) >= ML_THREADS ? 1 : ML_THREADS >> lg;
    const int64_t groups = ((int64_t)nQ + G - 1) / G;
    hipLaunchKernelGGL(search_merge_lists_kernel, dim3((unsigned)groups), dim3(ML_THREADS), 0, (hipStream_t)stream,
                       (const uint32_t*)part_vals, part_idx, shard_stride, row0, nQ, S, k, lg, vals, idx);
    SC_LAUNCH_CHECK();
    return 0;
}
