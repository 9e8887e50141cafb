// Epilogue of the 256-row bf16 GEMM kernel (textual include of gemm256_bf16.hip).  Expects in scope:
//   p (sc_gemm_args), smem, lane, wave, wm, wn, TN, FN, ACT, DROP, RES, acc[8][FN] (transposed 16 x 16 fragments: a lane owns
//   row 16 mi + lane % 16 and columns 16 ni + 4 (lane / 16) + 0..3), cm0 / cn0 (tile origin), Rs, coff, drop_thr, drop_scale,
//   and last_par, BUF_BYTES, EPI_BYTES such that smem + last_par * BUF_BYTES + wave * EPI_BYTES is the wave's private 8 KiB.
            int el = lane;
            asm volatile("" : "+v"(el));
            float* Cw = (float*)(smem + last_par * BUF_BYTES + wave * EPI_BYTES);
            const bool transposed = (p.n_split >= 0) && (cn0 >= p.n_split);
            const int wn0 = cn0 + wn * TN;                // wave's first column
            constexpr int CPR = TN / 8;                   // 8-column chunks per row
            constexpr int TNP = TN == 48 ? 52 : TN;       // LDS row pitch in floats (48: padded against bank conflicts)
            if (LN == 1) {
                // LayerNorm-folded A operand: acc = raw_row . W'^T  ->  y = rstd (acc - mean s_n) + c_n   (see the kernel's header)
                // the tile's statistics rows and column constants were brought into LDS during K-tile 0 (dma_ln): no global load here
                const float inv_k = 1.f / (float)p.K;
                const float* rowst = (const float*)(smem + LN_OFF_ROWST);
                const float* colc = (const float*)(smem + LN_OFF_COLC);
                float mu[8], rs[8];
#pragma unroll
                for (int mi = 0; mi < 8; ++mi) {
                    const int r = wm * 128 + mi * 16 + (el & 15);
                    const f32x4 t0 = *(const f32x4*)(rowst + r * 8), t1 = *(const f32x4*)(rowst + r * 8 + 4);
                    const float s1 = (t0[0] + t0[2]) + (t1[0] + t1[2]), s2 = (t0[1] + t0[3]) + (t1[1] + t1[3]);
                    const float mean = s1 * inv_k;
                    mu[mi] = mean;
                    rs[mi] = rsqrtf(fmaxf(s2 * inv_k - mean * mean, 0.f) + p.ln_eps);
                }
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) {
                    const int cl = wn * TN + ni * 16 + 4 * (el >> 4);        // column inside the tile (columns past N are never stored)
                    const f32x4 sv = *(const f32x4*)(colc + cl);
                    f32x4 cv = {0.f, 0.f, 0.f, 0.f};
                    if (bias) cv = *(const f32x4*)(colc + 256 + cl);
#pragma unroll
                    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = fmaf(rs[mi], fmaf(-mu[mi], sv[r], acc[mi][ni][r]), cv[r]);
                }
            }
            if (transposed) {
                // V^T store (QKV GEMM, columns >= n_split): passes of 64 rows (m) x 32 columns (n) staged as [n][64 m] so a
                // column's 64 consecutive frames leave as one full 128-B line; 16-B m-chunks XOR-swizzled by n & 15 (the 16
                // lanes of a fragment row group write the same m-chunk of 16 different n: 256-B stride otherwise)
                const int H = (p.N - p.n_split) / p.dh;
#pragma unroll
                for (int mh = 0; mh < 2; ++mh)
#pragma unroll
                    for (int ng = 0; ng < (FN + 1) / 2; ++ng) {
                        const int nfr = (FN - 2 * ng) < 2 ? (FN - 2 * ng) : 2;      // fragments (16 n each) in this pass
#pragma unroll
                        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                            for (int nj = 0; nj < 2; ++nj) {
                                if (nj >= nfr) continue;
                                f32x4 v = acc[mh * 4 + mi][ng * 2 + nj];
                                if (ACT == 1) {
                                    const f32x2 g0 = gelu_bf2(f32x2{v[0], v[1]}), g1 = gelu_bf2(f32x2{v[2], v[3]});
                                    v = f32x4{g0.x, g0.y, g1.x, g1.y};
                                }
                                if (ACT == 2) v = qgelu4(v);
                                const int ml = mi * 16 + (el & 15);
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int nl = nj * 16 + 4 * (el >> 4) + r;
                                    Cw[nl * 64 + (((ml >> 2) ^ (nl & 15)) << 2) + (ml & 3)] = v[r];
                                }
                            }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            if (it >= 2 * nfr) continue;
                            const int q = it * 64 + el;
                            const int nrow = q >> 3, mc = q & 7;
                            const int m = cm0 + wm * 128 + mh * 64 + mc * 8, n = wn0 + ng * 32 + nrow;
                            if (m < p.M && n < p.N) {
                                const f32x4 lo = *(const f32x4*)(Cw + nrow * 64 + (((2 * mc) ^ (nrow & 15)) << 2));
                                const f32x4 hi = *(const f32x4*)(Cw + nrow * 64 + (((2 * mc + 1) ^ (nrow & 15)) << 2));
                                const int nn = n - p.n_split, hh = nn / p.dh, d = nn % p.dh;
                                uint16_t* dst;
                                if (p.seg_chunk) {       // ragged rows: (first row, pitch) of the utterance that owns this 8-row chunk
                                    const int2 sg = *(const int2*)(p.seg_chunk + 4 * (m >> 3));
                                    dst = p.Ct + (int64_t)(p.N - p.n_split) * sg.x + (int64_t)nn * sg.y + (m - sg.x);
                                } else {
                                    const int b = m / p.R, t = m % p.R;
                                    dst = p.Ct + (((int64_t)b * H + hh) * p.dh + d) * p.R + t;
                                }
                                uint4 o;
                                o.x = pack2bf(lo[0], lo[1]); o.y = pack2bf(lo[2], lo[3]);
                                o.z = pack2bf(hi[0], hi[1]); o.w = pack2bf(hi[2], hi[3]);
                                *(uint4*)dst = o;
                            }
                        }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                    }
            } else if (RES) {
                // ---- tiles with a residual: staged through the wave's private 8 KiB of buffer last_par, 32 rows a pass, so that
                // every store instruction writes FULL 128-byte rows (non-temporal: the output is the next residual stream and is
                // read next by a LayerNorm pass) and every residual load is a full row too.  Measured against the register-direct
                // form below on the out_proj / fc2 shapes: 60 vs 76 us / 138 vs 160 us.  Fragments go in as 16-byte chunks (a lane
                // owns 4 consecutive columns of one row), chunk index XOR row & 15: conflict-free writes and reads.
                // LN = 2: the residual may be a RAW row, normalised here (p.res_stats), and the sum / sum of squares of the stored
                // bf16 values leave per row as well: lane -> LDS [row][chunk], lanes 0..31 add a row's chunks in order.
                f32x2* statL = (f32x2*)(smem + LDS_BYTES) + wave * 128;
                const float* rowst = (const float*)(smem + LN_OFF_ROWST);
                const float* colc = (const float*)(smem + LN_OFF_COLC);
                f32x2* statW = (f32x2*)(smem + LDS_BYTES + STATL_BYTES) + wave * 128;
                const float inv_n = 1.f / (float)p.N;
#pragma unroll
                for (int ms = 0; ms < 4; ++ms) {
                    const int wm0 = cm0 + wm * 128 + ms * 32;
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < FN; ++ni) {
                            f32x4 v = acc[ms * 2 + mi][ni];
                            if (ACT == 1) {
                                const f32x2 g0 = gelu_bf2(f32x2{v[0], v[1]}), g1 = gelu_bf2(f32x2{v[2], v[3]});
                                v = f32x4{g0.x, g0.y, g1.x, g1.y};
                            }
                            if (ACT == 2) v = qgelu4(v);
                            const int ml = mi * 16 + (el & 15), ch = ni * 4 + (el >> 4);
                            *(f32x4*)(Cw + ml * 64 + ((ch ^ (ml & 15)) << 2)) = v;
                        }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int it = 0; it < CPR / 2; ++it) {
                        const int q = it * 64 + el;
                        const int row = q / CPR, cc = q % CPR;
                        const int m = wm0 + row, n = wn0 + cc * 8;
                        float st1 = 0.f, st2 = 0.f;
                        if (m < p.M && n + 8 <= p.N) {
                            const f32x4 lo = *(const f32x4*)(Cw + row * 64 + (((2 * cc) ^ (row & 15)) << 2));
                            const f32x4 hi = *(const f32x4*)(Cw + row * 64 + (((2 * cc + 1) ^ (row & 15)) << 2));
                            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                            if (DROP) {
                                const uint32_t keep = sc_keep8((uint32_t)m * (uint32_t)p.N + (uint32_t)n, p.drop_seed, drop_thr);
#pragma unroll
                                for (int e = 0; e < 8; ++e) v[e] = (keep >> e) & 1u ? v[e] * drop_scale : 0.f;
                            }
                            if (Rs) {
                                const uint4 rv = *(const uint4*)(Rs + (int64_t)m * p.ldr + n);
                                float r[8] = {bflo(rv.x), bfhi(rv.x), bflo(rv.y), bfhi(rv.y), bflo(rv.z), bfhi(rv.z), bflo(rv.w), bfhi(rv.w)};
                                if (LN == 2 && p.res_stats) {
                                    const int rl = wm * 128 + ms * 32 + row;             // statistics row / constants from LDS (dma_ln)
                                    const f32x4 t0 = *(const f32x4*)(rowst + rl * 8), t1 = *(const f32x4*)(rowst + rl * 8 + 4);
                                    const float s1 = (t0[0] + t0[2]) + (t1[0] + t1[2]), s2 = (t0[1] + t0[3]) + (t1[1] + t1[3]);
                                    const float mean = s1 * inv_n;
                                    const float rstd = rsqrtf(fmaxf(s2 * inv_n - mean * mean, 0.f) + p.ln_eps);
                                    const int cl = wn * TN + cc * 8;
                                    const f32x4 ga = *(const f32x4*)(colc + cl), gb = *(const f32x4*)(colc + cl + 4);
                                    const f32x4 ba = *(const f32x4*)(colc + 256 + cl), bb = *(const f32x4*)(colc + 256 + cl + 4);
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        r[e] = fmaf((r[e] - mean) * rstd, ga[e], ba[e]);
                                        r[4 + e] = fmaf((r[4 + e] - mean) * rstd, gb[e], bb[e]);
                                    }
                                }
#pragma unroll
                                for (int e = 0; e < 8; ++e) v[e] += r[e];
                            }
                            if (p.out_f32) {
                                float* C = (float*)p.C + coff + (int64_t)m * p.ldc + n;
                                *(f32x4*)C = f32x4{v[0], v[1], v[2], v[3]};
                                *(f32x4*)(C + 4) = f32x4{v[4], v[5], v[6], v[7]};
                            } else {
                                uint16_t* C = (uint16_t*)p.C + coff + (int64_t)m * p.ldc + n;
                                uint4 o;
                                o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]);
                                o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
                                if (p.reserved & 1) {
                                    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
                                    __builtin_nontemporal_store(u32x4{o.x, o.y, o.z, o.w}, (u32x4*)C);
                                } else {
                                    *(uint4*)C = o;
                                }
                                if (LN == 2) {           // statistics of what was STORED (the consumer multiplies these bf16 values)
                                    const float x[8] = {bflo(o.x), bfhi(o.x), bflo(o.y), bfhi(o.y), bflo(o.z), bfhi(o.z), bflo(o.w), bfhi(o.w)};
#pragma unroll
                                    for (int e = 0; e < 8; ++e) {
                                        st1 += x[e];
                                        st2 = fmaf(x[e], x[e], st2);
                                    }
                                }
                            }
                        }
                        if (LN == 2) {           // the two chunks of an even / odd lane pair first (CPR is even: the pair shares its row)
                            st1 += __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(st1), 0xB1, 0xF, 0xF, true));
                            st2 += __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(st2), 0xB1, 0xF, 0xF, true));
                            if (!(el & 1)) statL[row * 4 + (cc >> 1)] = f32x2{st1, st2};
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    if (LN == 2) {
                        if (el < 32) {
                            float a1 = 0.f, a2 = 0.f;
#pragma unroll
                            for (int c2 = 0; c2 < CPR / 2; ++c2) {
                                const f32x2 t = statL[el * 4 + c2];
                                a1 += t.x;
                                a2 += t.y;
                            }
                            statW[ms * 32 + el] = f32x2{a1, a2};
                        }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            } else {
                // ---- register-direct epilogue.  Per output row m (one lane) and fragment PAIR (2p, 2p + 1): after
                // v_permlane16_swap the lanes of even lane-rows (lane / 16 = 0, 2) hold 8 consecutive columns of fragment 2p, the
                // odd ones 8 consecutive columns of fragment 2p + 1: GELU, dropout, residual and one 16-byte store per lane, with
                // no LDS round trip and no wait between fragments (the VALU stream of the GELU and the store issue overlap).
                // Tiles WITHOUT a residual only (GELU / conv / QKV / projection launches: 3 - 5 % faster than the staged form).
                const int g = el >> 4, l15 = el & 15;
                const int coff8 = ((g >> 1) << 3) + ((g & 1) << 4);
                // ACT 3 / 4 (round 4): erf-GELU fused with a second [M, N] bf16 operand at p.Ct, row stride ldc (sc_gemm_args.aux_mode):
                //   3  dual store: aux <- u = bf16(acc + bias), C <- gelu(u)        (FFN fc1 / conv layers of a differentiated encoder)
                //   4  C <- bf16(acc) * gelu'(aux)                                  (the input-gradient GEMM in front of that activation)
                // the same arithmetic on the same rounded values as GEMM + sc_act_bf16 (and as the 128-row tiles): bit-identical
                auto finish8 = [&](float (&v)[8], int m, int n) {
                    if (m < p.M && n + 8 <= p.N) {
                        if (ACT >= 3) {
                            uint16_t* X = p.Ct + coff + (int64_t)m * p.ldc + n;
                            uint4 r;
                            r.x = pack2bf(v[0], v[1]); r.y = pack2bf(v[2], v[3]); r.z = pack2bf(v[4], v[5]); r.w = pack2bf(v[6], v[7]);
                            const float rr[8] = {bflo(r.x), bfhi(r.x), bflo(r.y), bfhi(r.y), bflo(r.z), bfhi(r.z), bflo(r.w), bfhi(r.w)};
                            if (ACT == 3) {
                                *(uint4*)X = r;
#pragma unroll
                                for (int e = 0; e < 8; e += 2) {
                                    const f32x2 g2 = gelu_bf2(f32x2{rr[e], rr[e + 1]});
                                    v[e] = g2.x; v[e + 1] = g2.y;
                                }
                            } else {
                                const uint4 uu = *(const uint4*)X;
                                const float u8[8] = {bflo(uu.x), bfhi(uu.x), bflo(uu.y), bfhi(uu.y), bflo(uu.z), bfhi(uu.z), bflo(uu.w), bfhi(uu.w)};
                                // round 6: the derivative on PAIRS (gelu_grad_as2: packed fp32 polynomial / squarings, the same operations in the
                                // same order as the scalar form => the same bits; the scalar calls compiled to 18 VALU instructions per element)
#pragma unroll
                                for (int e = 0; e < 8; e += 2) {
                                    const f32x2 d2 = gelu_grad_as2(f32x2{u8[e], u8[e + 1]});
                                    v[e] = rr[e] * d2.x;
                                    v[e + 1] = rr[e + 1] * d2.y;
                                }
                            }
                        }
                        if (DROP) {                      // train-mode dropout before the residual add (F.dropout semantics)
                            const uint32_t keep = sc_keep8((uint32_t)m * (uint32_t)p.N + (uint32_t)n, p.drop_seed, drop_thr);
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = (keep >> e) & 1u ? v[e] * drop_scale : 0.f;
                        }
                        if (p.out_f32) {
                            float* C = (float*)p.C + coff + (int64_t)m * p.ldc + n;
                            *(f32x4*)C = f32x4{v[0], v[1], v[2], v[3]};
                            *(f32x4*)(C + 4) = f32x4{v[4], v[5], v[6], v[7]};
                        } else {
                            uint16_t* C = (uint16_t*)p.C + coff + (int64_t)m * p.ldc + n;
                            uint4 o;
                            o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]);
                            o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
                            *(uint4*)C = o;              // plain stores: the L2 merges a row's two 64-byte halves
                        }
                    }
                };
#pragma unroll
                for (int mi = 0; mi < 8; ++mi) {
                    const int m = cm0 + wm * 128 + mi * 16 + l15;
#pragma unroll
                    for (int pr = 0; pr < FN / 2; ++pr) {
                        f32x4 Fv = acc[mi][2 * pr], Gv = acc[mi][2 * pr + 1];
                        if (ACT == 1) {
                            const f32x2 a0 = gelu_bf2(f32x2{Fv[0], Fv[1]}), a1 = gelu_bf2(f32x2{Fv[2], Fv[3]});
                            const f32x2 b0 = gelu_bf2(f32x2{Gv[0], Gv[1]}), b1 = gelu_bf2(f32x2{Gv[2], Gv[3]});
                            Fv = f32x4{a0.x, a0.y, a1.x, a1.y};
                            Gv = f32x4{b0.x, b0.y, b1.x, b1.y};
                        }
                        if (ACT == 2) {
                            Fv = qgelu4(Fv);
                            Gv = qgelu4(Gv);
                        }
                        float v[8];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {    // odd lane-rows of F <-> even lane-rows of G
                            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(Fv[r]), __float_as_uint(Gv[r]), false, false);
                            v[r] = __uint_as_float(sw[0]);
                            v[4 + r] = __uint_as_float(sw[1]);
                        }
                        finish8(v, m, wn0 + pr * 32 + coff8);
                    }
                    if ((FN & 1) && (mi & 1)) {
                        // 192-wide tiles: the odd (third) fragment is paired ACROSS two row blocks - after the exchange the even
                        // lane-rows hold 8 consecutive columns of row block mi - 1, the odd ones 8 consecutive columns of row
                        // block mi: 16-byte stores here too
                        f32x4 Fv = acc[mi - 1][FN - 1], Gv = acc[mi][FN - 1];
                        if (ACT == 1) {
                            const f32x2 a0 = gelu_bf2(f32x2{Fv[0], Fv[1]}), a1 = gelu_bf2(f32x2{Fv[2], Fv[3]});
                            const f32x2 b0 = gelu_bf2(f32x2{Gv[0], Gv[1]}), b1 = gelu_bf2(f32x2{Gv[2], Gv[3]});
                            Fv = f32x4{a0.x, a0.y, a1.x, a1.y};
                            Gv = f32x4{b0.x, b0.y, b1.x, b1.y};
                        }
                        if (ACT == 2) {
                            Fv = qgelu4(Fv);
                            Gv = qgelu4(Gv);
                        }
                        float v[8];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(Fv[r]), __float_as_uint(Gv[r]), false, false);
                            v[r] = __uint_as_float(sw[0]);
                            v[4 + r] = __uint_as_float(sw[1]);
                        }
                        finish8(v, m - ((g & 1) ? 0 : 16), wn0 + (FN - 1) * 16 + ((g >> 1) << 3));
                    }
                }
            }
