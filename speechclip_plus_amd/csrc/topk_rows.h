// Per-row top-k (k <= 32) over an fp32 score row by one wave (gfx950): ONE definition for sc_topk_rows_f32 (topk.hip) and
// sc_topk_rows_filtered_f32 (search_filter.hip), which differ in the filter policy only.
//
// A lane owns every 64th group of four columns - a 16-byte load when the row base is 16-byte aligned and the pitch a multiple of four
// floats (VEC), four element loads 64 columns apart otherwise - and walks them in increasing column order.  It keeps its four best as
// (sortable key, column) in NAMED registers (a runtime-indexed register array would go to scratch), inserted by an unrolled strict
// compare-exchange: strict + increasing columns = the lower column stays in front among equal values.  A group is first tested
// against the lane's fourth-best as FLOATS (!(v <= t): one compare per element; NaN and an unfilled list fail it on purpose) and only
// a group with a candidate pays for keys and insertion.  The wave then pops the global best k times: a 64-lane maximum over the
// words key << 32 | ~column.  Four per lane is not a bound on the answer: a lane whose list runs empty while it still owns unlisted
// columns re-scans ITS columns for the next four that rank after its last popped pair before the next pop (rare on continuous
// scores - k of 64 lanes' best - and exact on tie-heavy rows).  Every score is read once (re-scans aside) -> bandwidth-bound; the k
// values are re-read at the end so the caller gets the matrix's own bits (-0, NaN payloads; a real -inf keeps its column).
//
// Filter policy: ``bool admissible(int col, bool enters) const`` for a column < V.  ``enters`` is false when the column's key would
// leave the lane's list as it is, and the answer is then irrelevant: a policy that reads memory returns without reading.
#pragma once
#include "search_common.h"

// every column is admissible: an empty object, and the test folds away
struct NoRowFilter {
    __device__ __forceinline__ constexpr bool admissible(int, bool) const { return true; }
};

// search_filter.hip's rule on one row: live is NULL or live[col] != 0, and the ids are NULL or g_ids[col] != qid.  A column's id and
// live byte are read only once its key would enter the list: for candidates, not for every score
struct RowFilter {
    const int64_t* g_ids;    // [V] or NULL
    const uint8_t* live;     // [V] or NULL
    int64_t qid;             // this row's id (g_ids != NULL)

    __device__ __forceinline__ bool admissible(int col, bool enters) const {
        bool ok = enters;
        if (ok && live) ok = live[col] != 0;
        if (ok && g_ids) ok = g_ids[col] != qid;
        return ok;
    }
};

struct Top4 {
    uint32_t k0, k1, k2, k3;     // keys, best first; TK_EMPTY = no entry
    int c0, c1, c2, c3;
    float thr;

    __device__ __forceinline__ void clear() {
        k0 = k1 = k2 = k3 = TK_EMPTY;
        c0 = c1 = c2 = c3 = -1;
        thr = tk_threshold(TK_EMPTY);
    }
    // strict: an equal key stays behind the entries already listed (they have lower columns)
    __device__ __forceinline__ void insert(uint32_t key, int col) {
        const bool g0 = key > k0, g1 = key > k1, g2 = key > k2, g3 = key > k3;
        k3 = g2 ? k2 : (g3 ? key : k3);  c3 = g2 ? c2 : (g3 ? col : c3);
        k2 = g1 ? k1 : (g2 ? key : k2);  c2 = g1 ? c1 : (g2 ? col : c2);
        k1 = g0 ? k0 : (g1 ? key : k1);  c1 = g0 ? c0 : (g1 ? col : c1);
        k0 = g0 ? key : k0;              c0 = g0 ? col : c0;
    }
    __device__ __forceinline__ void pop() {
        k0 = k1; k1 = k2; k2 = k3; k3 = TK_EMPTY;
        c0 = c1; c1 = c2; c2 = c3; c3 = -1;
        thr = tk_threshold(TK_EMPTY);
    }
};

// columns of group g of a lane, in increasing order: VEC - the 16-byte word lane + 64 g; else four elements 64 columns apart
template <bool VEC>
__device__ __forceinline__ int tk_col(int lane, int g, int j) {
    return VEC ? 4 * (lane + 64 * g) + j : lane + 64 * (4 * g + j);
}

template <bool VEC>
__device__ __forceinline__ void tk_load(const float* __restrict__ row, int lane, int g, float (&a)[4]) {
    if (VEC) {
        const f32x4 v = *(const f32x4*)(row + tk_col<true>(lane, g, 0));
        a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = row[tk_col<false>(lane, g, j)];
    }
}

// one group of four columns into the list.  REFILL: only admissible pairs that rank after (lk, lc), counted in ``seen``
template <bool VEC, bool REFILL, class Filter>
__device__ __forceinline__ void tk_group(Top4& t, const Filter& f, const float (&a)[4], int lane, int g, int nvalid, uint32_t lk, int lc,
                                         int& seen) {
    if (!REFILL && nvalid == 4 && a[0] <= t.thr && a[1] <= t.thr && a[2] <= t.thr && a[3] <= t.thr) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t key = tk_key(a[j]);
        const int col = tk_col<VEC>(lane, g, j);
        bool take = j < nvalid;
        if (REFILL) take = take && (key < lk || (key == lk && col > lc));
        if (take) take = f.admissible(col, REFILL || key > t.k3);    // not REFILL: any other key would leave the list as it is
        if (REFILL) seen += take ? 1 : 0;
        if (take) t.insert(key, col);
    }
    t.thr = tk_threshold(t.k3);
}

// all columns of this lane, in increasing order, four groups of loads in flight
template <bool VEC, bool REFILL, class Filter>
__device__ __forceinline__ void tk_scan(Top4& t, const Filter& f, const float* __restrict__ row, int V, int lane, uint32_t lk, int lc,
                                        int& seen) {
    int g = 0;
    for (; tk_col<VEC>(lane, g + 3, 3) < V; g += 4) {
        float a0[4], a1[4], a2[4], a3[4];
        tk_load<VEC>(row, lane, g, a0);
        tk_load<VEC>(row, lane, g + 1, a1);
        tk_load<VEC>(row, lane, g + 2, a2);
        tk_load<VEC>(row, lane, g + 3, a3);
        tk_group<VEC, REFILL>(t, f, a0, lane, g, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, f, a1, lane, g + 1, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, f, a2, lane, g + 2, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, f, a3, lane, g + 3, 4, lk, lc, seen);
    }
    for (; tk_col<VEC>(lane, g, 0) < V; ++g) {
        float a[4];
        int nvalid = 4;
        if (tk_col<VEC>(lane, g, 3) < V) {
            tk_load<VEC>(row, lane, g, a);
        } else {           // the row's last columns: element loads, nothing at or past V is touched
            nvalid = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = tk_col<VEC>(lane, g, j);
                const bool ok = c < V;
                a[j] = ok ? row[c] : 0.f;
                nvalid += ok ? 1 : 0;      // columns increase with j: the valid ones are the first nvalid
            }
        }
        tk_group<VEC, REFILL>(t, f, a, lane, g, nvalid, lk, lc, seen);
    }
}

// One wave selects the k best admissible columns of ``row`` into vals[0 .. k) / idx[0 .. k), best first, -inf / -1 behind the last
template <bool VEC, class Filter>
__device__ __forceinline__ void topk_select_row(const float* __restrict__ row, int V, int k, int lane, const Filter& f,
                                                float* __restrict__ vals, int32_t* __restrict__ idx) {
    Top4 t;
    t.clear();
    int seen = 0;
    tk_scan<VEC, false>(t, f, row, V, lane, 0u, 0, seen);
    // columns this lane owns (admissible or not): more than the list holds -> an empty list is not the end of the lane
    const int owned = VEC ? ((V + 3) / 4 > lane ? 4 * (((V + 3) / 4 - lane + 63) / 64) : 0) : (V > lane ? (V - lane + 63) / 64 : 0);
    bool more = owned > 4;
    int out_c = -1;
    for (int p = 0; p < k; ++p) {
        const uint64_t mine = t.k0 == TK_EMPTY ? 0ull : tk_word(t.k0, t.c0);
        const uint64_t best = wave_max_u64(mine);
        if (best == 0ull) break;                             // fewer than k admissible columns: wave-uniform
        if (lane == p) out_c = tk_word_col(best);
        if (mine == best) {                                  // columns are unique: exactly one lane
            const uint32_t lk = t.k0;
            const int lc = t.c0;
            t.pop();
            if (t.k0 == TK_EMPTY && more) {
                int cnt = 0;
                tk_scan<VEC, true>(t, f, row, V, lane, lk, lc, cnt);
                more = cnt > 4;
            }
        }
    }
    if (lane < k) {
        vals[lane] = out_c >= 0 ? row[out_c] : -INFINITY;    // the matrix's own bits; a real -inf keeps its column
        idx[lane] = out_c;
    }
}
