// Retrieval ranks (gfx950): for every row of A and every row of B, how many candidates of the other side rank ahead of its best
// correct candidate - the one integer per query that recall@k, median rank and mean rank are made of - produced in the epilogue of the
// split-bf16 score GEMM.  The [nA, nB] score matrix never exists in memory.  One kernel serves a whole gallery in one call
// (sc_rank_counts_bf16) and a gallery given as a list of (A range, B range) pairs - shards on this device, or the ranges of the ranks
// of a process group - that may have removed rows (sc_rank_best_bf16, sc_rank_ahead_bf16).
//   replaces: the sort-and-look-up of avssl/module/retrieval.py:45-121 (and the half dozen [nA, nB] temporaries a masked-maximum form
//             of it needs per direction) on the scores of avssl/model/kwClip.py:447-482, and the gather of every rank's embeddings
//             onto one device the reference's ``dp`` strategy did before it.
//
// Scores: csrc/search.hip's, to the bit - the same code.  A is the side-0 three-way split sc_split3_bf16 writes, B the side-1 split, rows
// padded to 128, K6 = 6 Ep columns; a score is the fp32 sum of the six K-blocks, K-tiles in increasing order: search_tile.h's tile, with
// its grid of row tiles x S slabs of column tiles (TileBlock).
//
// The pair (i, j) is CORRECT iff a_ids[i] == b_ids[j].  One 128 x 128 score tile serves both directions: its rows for A -> B, its columns
// for B -> A.  Two phases of one kernel body (template parameter PHASE), both over the same K loop, so the score compared in the second
// is bit for bit the score that produced ``best`` in the first:
//   PHASE 0, best:   per row the largest key (search_common.h's tk_key: float order, -0 == +0, every NaN on top) over correct, non-NaN
//                    columns; per column the same over correct, non-NaN rows.  Combined across tiles with atomicMax on a uint32 key
//                    per row / per column; key 0 = no correct non-NaN candidate.  A tile whose 128 + 128 ids hold no matching pair
//                    (every thread compares its column's id with half of the rows' ids in LDS, one workgroup-wide OR) contributes
//                    nothing and is skipped BEFORE its K loop: with few captions per image nearly all tiles are, and this launch
//                    takes 0.18 ms next to the second's 1.81 ms at 25 000 x 5 000 x 768 (docs/rounds/r14_ranks.md).
//   PHASE 1, count:  READS best_a / best_b; ahead_a[i] += #{j : s_ij > best_i} + #{j not correct : s_ij == best_i or s_ij is NaN},
//                    and the mirror image per column, compared on keys.  On keys that is: a correct candidate counts iff
//                    best < key < NaN, a wrong one iff key >= best (ahead_of).
//
// Why two phases, and the accumulate protocol.  ``ahead`` is counted against a query's best correct key, and that key must be final
// over ALL of the other side before any pair counts.  Both phases only ACCUMULATE into the caller's best_a / best_b / ahead_a /
// ahead_b (atomicMax, atomicAdd), which the caller zeroes once.  sc_rank_counts_bf16 launches the phases back to back on one pair.
// For a list of pairs the caller calls sc_rank_best_bf16 for every pair (between ranks: an all-reduce(MAX) of the row keys goes
// here), then sc_rank_ahead_bf16 for every pair.  A score depends only on its row of A, its row of B and the fixed K order, so the
// sum over the pairs is bit for bit what one call on the whole gallery gives.
//
// FILTER (template parameter; b_live != NULL): column j takes part iff b_live[j] != 0.  A dead column is no candidate of any row
// and no query of the column direction: it enters no maximum, no count, no ballot and no tile-skip test, and nothing is written to
// best_b[j] / ahead_b[j].  FILTER = false is the arithmetic of the whole gallery; sc_rank_counts_bf16 always runs it.
//
// Epilogue: the accumulators go to the LDS tile (over the staging ring) as KEYS.  Row direction: a wave owns 32 rows, a lane reads
// columns lane and lane + 64 of a row (conflict free); a row's count is two ballots and two scalar pop-counts, kept by lane (row & 31)
// in a register across the column tiles of the slab and added to ahead_a once, after the last tile.  Column direction: thread = column
// tid & 127 over rows 64 (tid >> 7) .. + 63 (consecutive lanes on consecutive banks; the rows' ids and best keys are LDS broadcasts);
// the two halves meet in LDS and threads 0 .. 127 issue one int32 atomic per column per tile - one lane per consecutive column, 256
// contiguous bytes per wave instruction.  Rows >= nA and columns >= nB are excluded by their index.
//
// Safety, held throughout:
//   - only integer atomicMax / atomicAdd from vector lanes, and plain C++ stores (to LDS); the result is bitwise reproducible and
//     independent of S and of the order of the calls;
//   - no address is computed from a score, a key, an id or a mask byte: they are compared, never used as an index;
//   - b_live, b_ids, best_b, ahead_b are indexed by j < nB only; a_ids, best_a, ahead_a by i < nA only; a_split / b_split rows are
//     padded to 128, which the tile's DMA relies on;
//   - every buffer is the caller's; nothing is allocated; every argument check comes before the first launch; nA == 0 or nB == 0
//     returns 0 without a launch.
#include "search_tile.h"

#include <algorithm>

namespace {

constexpr int SIDE_BYTES = BM * 8 + BM * 4 + 2 * BN * 4;   // ids and best keys of the 128 rows, the two halves' column partials
constexpr int LDS_BYTES = RING_BYTES + SIDE_BYTES;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// does a candidate with key ``key`` rank ahead of a best correct candidate with key ``best``?
__device__ __forceinline__ bool ahead_of(uint32_t key, uint32_t best, bool correct) {
    return correct ? (key > best && key != TK_NAN) : key >= best;
}

struct RankArgs {
    const uint16_t* a;       // [roundup(nA, 128), K6] side-0 split
    const uint16_t* b;       // [roundup(nB, 128), K6] side-1 split
    const int64_t* a_ids;    // [nA]
    const int64_t* b_ids;    // [nB]
    const uint8_t* b_live;   // [nB] or NULL (FILTER = false)
    int nA, nB, K6, S, tiles;
    uint32_t* best_a;        // [nA] keys: written by PHASE 0, read by PHASE 1
    uint32_t* best_b;        // [nB]
    int32_t* ahead_a;        // [nA] PHASE 1 only
    int32_t* ahead_b;        // [nB]
};

template <int PHASE, bool FILTER>
__global__ __launch_bounds__(256) void rank_kernel(const RankArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const TileBlock blk(p.nA, p.nB, p.tiles);
    const int m0 = blk.m0;
    const ScoreTile tile(p.a, p.b, m0, p.K6);
    const int lane = tile.lane, wave = tile.wave;

    uint32_t* const Ks = (uint32_t*)smem;                               // [BM][BN] keys of the tile's scores
    int64_t* const aid_s = (int64_t*)(smem + RING_BYTES);               // [BM] ids of the tile's rows
    uint32_t* const abest_s = (uint32_t*)(smem + RING_BYTES + BM * 8);  // [BM] their best keys (PHASE 1)
    uint32_t* const colpart = abest_s + BM;                             // [2][BN] the two row halves' column results

    const int rows_valid = min(BM, p.nA - m0);                         // >= 1: rows of this tile that exist
    if (tid < BM) {
        const bool v = tid < rows_valid;
        aid_s[tid] = v ? p.a_ids[m0 + tid] : 0;
        if (PHASE == 1) abest_s[tid] = v ? p.best_a[m0 + tid] : 0u;
    }
    __syncthreads();

    // column direction: this thread's column of the tile and its half of the rows
    const int c = tid & (BN - 1);
    const int cr0 = (tid >> 7) * 64, cr1 = min(cr0 + 64, rows_valid);
    // row direction: this wave's rows; lane rr keeps the result of row wave * 32 + rr across the tiles of the slab
    const int rows_here = min(32, p.nA - m0 - wave * 32);              // wave-uniform; <= 0: nothing to scan
    uint32_t row_acc = 0;

    for (int t = blk.t_begin; t < blk.t_end; ++t) {
        const int n0 = t * BN;
        // this thread's columns: do they exist, their ids (and best keys) and, under FILTER, their mask bytes - every load guarded by
        // the column's index alone, so that none waits for another, straight from global memory and in flight under the K loop
        const bool inc = n0 + c < p.nB, in0 = n0 + lane < p.nB, in1 = n0 + 64 + lane < p.nB;
        const int64_t bid_c = inc ? p.b_ids[n0 + c] : 0;
        const int64_t bid0 = in0 ? p.b_ids[n0 + lane] : 0, bid1 = in1 ? p.b_ids[n0 + 64 + lane] : 0;
        uint32_t bestc = 0;
        if (PHASE == 1 && inc) bestc = p.best_b[n0 + c];
        // does the column take part: it exists and, under FILTER, is live
        bool okc = inc, ok0 = in0, ok1 = in1;
        if (FILTER) {
            okc = inc && p.b_live[n0 + c] != 0;
            ok0 = in0 && p.b_live[n0 + lane] != 0;
            ok1 = in1 && p.b_live[n0 + 64 + lane] != 0;
        }
        if (PHASE == 0) {
            // no matching pair of ids among the rows and the columns that take part: nothing to take a maximum over
            int hit = 0;
            if (okc)
                for (int r = cr0; r < cr1; ++r) hit |= (int)(aid_s[r] == bid_c);
            if (!__syncthreads_or(hit)) continue;
        }

        f32x4 acc[FM][FN];
        tile.scores(smem, n0, acc);
        tile.store(Ks, acc, [](float s) { return tk_key(s); });      // the tile holds KEYS

        // ---- row direction: wave w scans rows 32 w .. 32 w + 31, a lane the columns lane and lane + 64 ---------------------
        for (int rr = 0; rr < rows_here; ++rr) {
            const int r = wave * 32 + rr;
            const uint32_t key0 = Ks[r * BN + lane], key1 = Ks[r * BN + 64 + lane];
            const int64_t aid = aid_s[r];
            const bool c0 = ok0 && aid == bid0, c1 = ok1 && aid == bid1;
            if (PHASE == 0) {
                const uint32_t m = wave_max_u32(max(c0 && key0 != TK_NAN ? key0 : 0u, c1 && key1 != TK_NAN ? key1 : 0u));
                if (lane == rr) row_acc = max(row_acc, m);
            } else {
                const uint32_t best = abest_s[r];
                const uint64_t m0b = __ballot(ok0 && ahead_of(key0, best, c0)), m1b = __ballot(ok1 && ahead_of(key1, best, c1));
                const uint32_t n = (uint32_t)(__popcll(m0b) + __popcll(m1b));
                if (lane == rr) row_acc += n;
            }
        }
        // ---- column direction: thread = column c over its half of the rows that exist -------------------------------------------
        {
            uint32_t v = 0;
            for (int r = cr0; r < cr1; ++r) {
                const uint32_t key = Ks[r * BN + c];
                const bool cor = aid_s[r] == bid_c;
                if (PHASE == 0) v = max(v, cor && key != TK_NAN ? key : 0u);
                else v += ahead_of(key, bestc, cor) ? 1u : 0u;
            }
            colpart[(tid >> 7) * BN + c] = v;
        }
        __syncthreads();   // the halves meet; and every read of the key tile is done: the next tile's DMA may overwrite it
        if (tid < BN && okc) {                                         // a dead column's slots are not touched
            const uint32_t v0 = colpart[c], v1 = colpart[BN + c];
            if (PHASE == 0) {
                const uint32_t m = max(v0, v1);
                if (m) atomicMax(p.best_b + n0 + c, m);
            } else {
                if (v0 + v1) atomicAdd(p.ahead_b + n0 + c, (int32_t)(v0 + v1));
            }
        }
        // colpart is written again only behind the next tile's K-loop barriers
    }

    // ---- this slab's share of every row, once -----------------------------------------------------------------------------------
    if (lane < rows_here && row_acc) {
        const int row = m0 + wave * 32 + lane;
        if (PHASE == 0) atomicMax(p.best_a + row, row_acc);
        else atomicAdd(p.ahead_a + row, (int32_t)row_acc);
    }
}

template <int PHASE, bool FILTER>
int launch(const RankArgs& a, int64_t nwg, hipStream_t stream) {
    static sc_lds_attr_once attr;
    if (hipError_t e = sc_set_max_lds_once(attr, rank_kernel<PHASE, FILTER>, LDS_BYTES); e != hipSuccess) {
        sc_set_error("hipFuncSetAttribute(rank): %s", hipGetErrorString(e));
        return -3;
    }
    hipLaunchKernelGGL((rank_kernel<PHASE, FILTER>), dim3((unsigned)nwg), dim3(256), LDS_BYTES, stream, a);
    SC_LAUNCH_CHECK();
    return 0;
}

// the argument checks of all three entries (``name``: the entry's own; ``counts``: does it write ahead_a / ahead_b) -> 0 with ``a``
// and the number of workgroups ``nwg`` filled in (nwg == 0: no pair, nothing to launch), or the failed check's code
int rank_args(const char* name, bool counts, const sc_bf16* a_split, const sc_bf16* b_split, const int64_t* a_ids, const int64_t* b_ids,
              const uint8_t* b_live, int32_t nA, int32_t nB, int32_t K6, int32_t S, uint32_t* best_a, uint32_t* best_b, int32_t* ahead_a,
              int32_t* ahead_b, RankArgs& a, int64_t& nwg) {
    nwg = 0;
    SC_CHECK(nA >= 0 && nB >= 0, "%s: nA >= 0, nB >= 0 (nA %d, nB %d)", name, nA, nB);
    SC_CHECK(K6 > 0 && K6 % 384 == 0, "%s: K6=%d must be 6 Ep with Ep a multiple of 64", name, K6);
    SC_CHECK(S >= 1, "%s: S >= 1 (S %d)", name, S);
    if (nA == 0 || nB == 0) return 0;                                 // no pair: nothing to accumulate
    const int64_t nM = ((int64_t)nA + BM - 1) / BM, nT = ((int64_t)nB + BN - 1) / BN;
    const int64_t tiles = (nT + S - 1) / S;                           // a slab past the last tile is empty: its workgroups add nothing
    SC_CHECK(a_split, "%s: null a_split", name);
    SC_CHECK(b_split, "%s: null b_split", name);
    SC_CHECK(a_ids, "%s: null a_ids", name);
    SC_CHECK(b_ids, "%s: null b_ids", name);
    SC_CHECK(best_a, "%s: null best_a", name);
    SC_CHECK(best_b, "%s: null best_b", name);
    if (counts) {
        SC_CHECK(ahead_a, "%s: null ahead_a", name);
        SC_CHECK(ahead_b, "%s: null ahead_b", name);
    }
    SC_CHECK(((uintptr_t)a_split % 16) == 0 && ((uintptr_t)b_split % 16) == 0, "%s: operands must be 16-byte aligned", name);
    SC_CHECK(((uintptr_t)a_ids % 8) == 0 && ((uintptr_t)b_ids % 8) == 0, "%s: ids must be 8-byte aligned", name);
    SC_CHECK(((uintptr_t)best_a % 4) == 0 && ((uintptr_t)best_b % 4) == 0 && ((uintptr_t)ahead_a % 4) == 0 && ((uintptr_t)ahead_b % 4) == 0,
             "%s: keys and counts must be 4-byte aligned", name);
    SC_CHECK(nM * S < ((int64_t)1 << 31), "%s: %lld workgroups", name, (long long)(nM * S));
    a.a = (const uint16_t*)a_split;
    a.b = (const uint16_t*)b_split;
    a.a_ids = a_ids; a.b_ids = b_ids; a.b_live = b_live;
    a.nA = nA; a.nB = nB; a.K6 = K6; a.S = S; a.tiles = (int)tiles;
    a.best_a = best_a; a.best_b = best_b; a.ahead_a = ahead_a; a.ahead_b = ahead_b;
    nwg = nM * S;
    return 0;
}

template <int PHASE>
int launch_live(const RankArgs& a, int64_t nwg, hipStream_t stream) {
    return a.b_live ? launch<PHASE, true>(a, nwg, stream) : launch<PHASE, false>(a, nwg, stream);
}

}  // namespace

extern "C" int sc_rank_best_bf16(const sc_bf16* a_split, const sc_bf16* b_split, const int64_t* a_ids, const int64_t* b_ids,
                                 const uint8_t* b_live, int32_t nA, int32_t nB, int32_t K6, int32_t S, uint32_t* best_a, uint32_t* best_b,
                                 void* stream) {
    RankArgs a;
    int64_t nwg;
    if (int rc = rank_args("sc_rank_best_bf16", false, a_split, b_split, a_ids, b_ids, b_live, nA, nB, K6, S, best_a, best_b, nullptr,
                           nullptr, a, nwg); rc != 0 || nwg == 0) return rc;
    return launch_live<0>(a, nwg, (hipStream_t)stream);
}

extern "C" int sc_rank_ahead_bf16(const sc_bf16* a_split, const sc_bf16* b_split, const int64_t* a_ids, const int64_t* b_ids,
                                  const uint8_t* b_live, int32_t nA, int32_t nB, int32_t K6, int32_t S, const uint32_t* best_a,
                                  const uint32_t* best_b, int32_t* ahead_a, int32_t* ahead_b, void* stream) {
    RankArgs a;
    int64_t nwg;
    if (int rc = rank_args("sc_rank_ahead_bf16", true, a_split, b_split, a_ids, b_ids, b_live, nA, nB, K6, S, (uint32_t*)best_a,
                           (uint32_t*)best_b, ahead_a, ahead_b, a, nwg); rc != 0 || nwg == 0) return rc;
    return launch_live<1>(a, nwg, (hipStream_t)stream);
}

extern "C" int sc_rank_counts_bf16(const sc_bf16* a_split, const sc_bf16* b_split, const int64_t* a_ids, const int64_t* b_ids, int32_t nA,
                                   int32_t nB, int32_t K6, int32_t S, uint32_t* best_a, uint32_t* best_b, int32_t* ahead_a, int32_t* ahead_b,
                                   void* stream) {
    RankArgs a;
    int64_t nwg;
    if (int rc = rank_args("sc_rank_counts_bf16", true, a_split, b_split, a_ids, b_ids, nullptr, nA, nB, K6, S, best_a, best_b, ahead_a,
                           ahead_b, a, nwg); rc != 0 || nwg == 0) return rc;
    if (int rc = launch<0, false>(a, nwg, (hipStream_t)stream); rc != 0) return rc;
    return launch<1, false>(a, nwg, (hipStream_t)stream);
}
