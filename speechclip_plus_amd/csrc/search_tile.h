// The 128 x 128 bf16 score tile of the search family (gfx950): ONE definition for the list scan (search_scan.h) and rank.hip.
//
// Operands: row-major bf16 [rows padded to 128, K], K a multiple of 64 - the three-way splits sc_split3_bf16 writes (K = 6 Ep) or the
// plain bf16 rows of sc_rows_bf16 (K = Ep).  A score is the fp32 sum over K on v_mfma_f32_16x16x32_bf16, K-tiles in increasing order,
// so it does not depend on the grid.  The K loop is the one of gemm_bf16.hip's 128 x 128 tile: 256 threads = 2 x 2 waves of 64 x 64,
// LDS-DMA staging into a two-stage ring, the 16-byte chunk index XOR ((row >> 1) & 7) applied on the global source address, one barrier
// per K-tile.  After the K loop the accumulators go to LDS over the ring, 128 x 128 32-bit words, through a per-element transform.
//
// Grid: row tiles x S column slabs; a slab is ``tiles`` whole column tiles and a workgroup walks them in increasing column order.
#pragma once
#include "search_common.h"

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int ROWB = BK * 2;                        // bytes per LDS tile row
constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB;
constexpr int RING_BYTES = 2 * (A_BYTES + B_BYTES);
static_assert(RING_BYTES == BM * BN * 4, "the 32-bit score tile lies exactly over the two-stage ring");
constexpr int TM = 64, TN = 64, FM = 4, FN = 4;     // per-wave tile, 16 x 16 fragments
constexpr int A_INST = BM / 32, B_INST = BN / 32;   // DMA instructions per wave and operand: 8 rows of 128 bytes each

// block -> (row tile, slab): XCD remap (bijective; blocks b, b + 8, ... share an L2), then row tiles fastest, so the workgroups of a
// slab walk the same column tiles side by side.  A slab past the last column tile is empty: t_begin == t_end.
struct TileBlock {
    int slab, m0, t_begin, t_end;

    __device__ __forceinline__ TileBlock(int n_rows, int n_cols, int tiles) {
        const int nM = (n_rows + BM - 1) / BM;
        const int nT = (n_cols + BN - 1) / BN;
        const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
        slab = L / nM;
        m0 = (L - slab * nM) * BM;
        t_begin = min(nT, slab * tiles);
        t_end = min(nT, t_begin + tiles);
    }
};

// Per-lane state of the K loop: what does not change from one column tile to the next.
struct ScoreTile {
    int lane, wave, wm, wn;
    int K, nk;
    const uint16_t* b;
    const uint16_t* a_src[A_INST];                  // DMA sources of the row tile (the swizzle lives in the source address)
    int a_off[FM][2], b_off[FN][2];                 // byte offsets of this lane's MFMA fragments in a staged tile

    __device__ __forceinline__ ScoreTile(const uint16_t* a, const uint16_t* b_, int m0, int K_) : K(K_), nk(K_ / BK), b(b_) {
        lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        wm = wave >> 1;
        wn = wave & 1;
#pragma unroll
        for (int i = 0; i < A_INST; ++i) {
            const int row = (i * 4 + wave) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            a_src[i] = a + (int64_t)(m0 + row) * K + c * 8;           // rows are padded to 128: in bounds
        }
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
            const int row = wm * TM + mi * 16 + (lane & 15);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) a_off[mi][kk] = row * ROWB + (((kk * 4 + (lane >> 4)) ^ ((row >> 1) & 7)) << 4);
        }
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
            const int row = wn * TN + ni * 16 + (lane & 15);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) b_off[ni][kk] = row * ROWB + (((kk * 4 + (lane >> 4)) ^ ((row >> 1) & 7)) << 4);
        }
    }

    __device__ __forceinline__ void stage(char* smem, const uint16_t* (&b_src)[B_INST], int buf, int kt) const {
        char* const As = smem;
        char* const Bs = smem + 2 * A_BYTES;
#pragma unroll
        for (int i = 0; i < A_INST; ++i) glds16(a_src[i] + kt * BK, As + buf * A_BYTES + (i * 4 + wave) * 1024);
#pragma unroll
        for (int i = 0; i < B_INST; ++i) glds16(b_src[i] + kt * BK, Bs + buf * B_BYTES + (i * 4 + wave) * 1024);
    }

    // acc = the scores of the row tile against columns n0 .. n0 + 127.  Every wave must be done with the LDS tile of the tile before;
    // returns behind the K loop's last barrier, so every wave is past the ring.
    __device__ __forceinline__ void scores(char* smem, int n0, f32x4 (&acc)[FM][FN]) const {
        const uint16_t* b_src[B_INST];
#pragma unroll
        for (int i = 0; i < B_INST; ++i) {
            const int row = (i * 4 + wave) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            b_src[i] = b + (int64_t)(n0 + row) * K + c * 8;           // rows are padded to 128: in bounds
        }
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

        stage(smem, b_src, 0, 0);
        __syncthreads();   // hipcc drains the DMA (vmcnt(0)) in front of the barrier
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) stage(smem, b_src, buf ^ 1, kt + 1);
            const char* as = smem + buf * A_BYTES;
            const char* bs = smem + 2 * A_BYTES + buf * B_BYTES;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 af[FM], bfr[FN];
#pragma unroll
                for (int mi = 0; mi < FM; ++mi) af[mi] = *(const bf16x8*)(as + a_off[mi][kk]);
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) bfr[ni] = *(const bf16x8*)(bs + b_off[ni][kk]);
#pragma unroll
                for (int mi = 0; mi < FM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < FN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
            }
            __syncthreads();
        }
    }

    // accumulators -> LDS tile tile[BM][BN] = f(score), over the ring; returns behind a barrier: every wave may read the whole tile
    template <class T, class F>
    __device__ __forceinline__ void store(T* tile, const f32x4 (&acc)[FM][FN], F&& f) const {
        static_assert(sizeof(T) == 4, "the LDS tile holds 32-bit words");
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
            const int nl = wn * TN + ni * 16 + (lane & 15);
#pragma unroll
            for (int mi = 0; mi < FM; ++mi) {
                const int ml = wm * TM + mi * 16 + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) tile[(ml + r) * BN + nl] = f(acc[mi][ni][r]);
            }
        }
        __syncthreads();
    }
};
