// rt_spec_scan_walk.inc -- the walk of length spectra over the march record and its stores: everything of spec_scan_tile
// (rt_spec_scan.hip) behind the per-block state, as text, so that the emission half of rt_spec_scan_ase_seeds.hip takes the
// same statements (rt_tile_rec.inc says why text and not a function template).
//
// A fragment of a function body.  Reads from the including scope: EMIS, BACKWARD, SF (= 0), LCH (= LSPEC_LCH); H, Q (Q->out.Iv:
// block jb of this walk is Iv + jb n_rays K), tab, stage, lane, L, S, K, Kp, n_rays, row0, rec, rrec, flags_steps, backward,
// exact_emis, sfk, f0_launch, blk_rays; the bits livem and seedm, which open_block(mseg) sets and whose seed factor
// (backward, gain-only) it returns; adds to negm and nanm.
// The stores of a staged column (flush_row) are the text both walks include: rt_spec_scan_tile.inc, SPEC_SCAN_FLUSH.
// Forward it opens every block first and then walks once per frequency batch; backward it opens the blocks of a chunk of
// LCH suffixes ahead of the chunk's walks.

    // a full tile and an even K: the pieces of a row leave as 16-byte stores
    const bool wide_ok = row0 + WAVE <= n_rays && (K & 1) == 0;
    // the lane's VEC values of block jb into column `col` of its staging row, the -2 / -3 scan on the way (Helper.h:582-587)
    auto stage_row = [&](const int col, const int jb, const double (&Iv)[VEC], const int kb) {
        const bool lv = ((livem >> jb) & 1u) != 0u;
        double *mine  = stage + lane * XS_ROW + col * VEC;
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            const double x = (lv && kb + v < K) ? Iv[v] : 0.0; // (the padding columns K .. Kp-1 are not part of the spectrum)
            negm |= x < 0.0 ? 1u << jb : 0u;
            nanm |= x != x ? 1u << jb : 0u;
            mine[v] = x;
        }
    };
    // column `col` of the 64 staging rows to block jb, frequencies kb .. kb + VEC - 1 (rt_spec_scan_tile.inc)
    auto flush_row = [&](const int col, const int jb, const int kb) {
        double *blk = Q->out.Iv + (size_t) jb * blk_rays * (size_t) K;
#define SPEC_SCAN_FLUSH
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_FLUSH
    };
    // Iv of a row from its accumulator: emission, the running value unless a NaN or an infinity was among the lineshape
    // values (0 * NaN on the CPU); gain-only, f0 f[4][k] exp(gl), the exponential skipped by a wave that has no use for it
    // (rt_tile_batch.inc)
    auto finish = [&](const double (&acc)[VEC], const unsigned wn, const double f0, const int kb, double (&Iv)[VEC]) {
        if (EMIS) {
#pragma unroll
            for (int v = 0; v < VEC; v++)
                Iv[v] = ((wn >> v) & 1u) ? __builtin_nan("") : acc[v];
        } else {
            bool need = f0 != 0.0;
#pragma unroll
            for (int v = 0; v < VEC; v++)
                need = need || acc[v] > 700.0 || acc[v] != acc[v];
#pragma unroll
            for (int v = 0; v < VEC; v++)
                Iv[v] = f0 * sfk[kb + v];
            if (__ballot(need) != 0ull) {
                double eg[VEC];
                exp_tab_vec(acc, tab, eg);
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    Iv[v] *= eg[v];
            }
        }
    };

    if (!BACKWARD) {
        // ---- forward: every block's state first, then one walk per frequency batch ----
#pragma unroll 1
        for (int j = 1; j <= L; j++)
            (void) open_block(j);
        const bool any_live = __ballot(livem != 0u) != 0ull; // (else nothing to integrate: the rows are zeros)
        for (int kb = 0; kb < K; kb += VEC) {
            double acc[VEC]; // emission: the running Iv; gain-only: the running gl
            double acc3[VEC]; // exact emission: the running Iv of the first two lengths in the arithmetic of the N = 3 plan (AseUpdate::apply_n3)
            unsigned wn = 0u; // emission, bit v: a NaN or infinity among frequency v's lineshape values so far
#pragma unroll
            for (int v = 0; v < VEC; v++)
                acc[v] = acc3[v] = 0.0;
#pragma unroll 1
            for (int j = 0; j < L; j++) {
                if (any_live) {
#pragma unroll 1
                    for (int t = 0; t < RT_N_SUB; t++) {
                        // one sub-segment: the SF = 0 text of rt_tile_batch.inc
                        int s = j * RT_N_SUB + t;
                        asm volatile("" : "+s"(s));
                        const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, flags_steps, backward);
                        const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                        const FVec w     = *reinterpret_cast<const FVec *>(row);
                        if (EMIS) {
                            const float g1 = sl.g, e1 = sl.e;
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                wn |= !(fabsf(w.v[v]) <= FLT_MAX) ? 1u << v : 0u;
                            if (fabsf(g1) >= RT_RS_MIN && fabsf(g1) <= H.gs_cap && !exact_emis) {
                                const double r1 = div_fast((double) e1, (double) g1);
                                ase_step(acc, g1, r1, w.v, tab);
                            } else if (g1 != 0.0f || e1 != 0.0f) {
#pragma unroll
                                for (int v = 0; v < VEC; v++)
                                    acc[v] = ase_update(acc[v], g1, e1, w.v[v], tab);
                                if (exact_emis && j < 2) { // (every update of the exact mode comes here: acc3 misses none)
#pragma unroll
                                    for (int v = 0; v < VEC; v++)
                                        acc3[v] = ase_update_factors(g1, e1, w.v[v], tab).apply_n3(acc3[v]);
                                }
                            }
                        } else {
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                acc[v] += (double) sl.g * (double) w.v[v];
                        }
                    }
                }
                // ---- the walk has reached length j + 1: row block j ----
                double Iv[VEC];
                finish(acc, wn, ((seedm >> j) & 1u) ? f0_launch : 0.0, kb, Iv);
                if (EMIS && exact_emis && j == 1) { // the rows of n = 3 (wn as above: the same slots)
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        Iv[v] = ((wn >> v) & 1u) ? __builtin_nan("") : acc3[v];
                }
                stage_row(j & (LCH - 1), j, Iv, kb);
                if ((j & (LCH - 1)) == LCH - 1 || j == L - 1) {
                    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                    for (int jj = j & ~(LCH - 1); jj <= j; jj++)
                        flush_row(jj & (LCH - 1), jj, kb);
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
    } else {
        // ---- backward: the suffixes in chunks of LCH start segments a0 .. a0 + LCH - 1 (start segment a is block L - 1 - a) ----
        for (int a0 = 0; a0 < L; a0 += LCH) {
            double f0[LCH];
#pragma unroll
            for (int i = 0; i < LCH; i++) {
                f0[i] = 0.0;
                if (a0 + i < L) {
                    const double f = open_block(L - (a0 + i));
                    if (!EMIS)
                        f0[i] = f;
                }
                // (one state after the other, as rt_step_rscan.hip takes them)
                asm volatile("" ::: "memory");
            }
            unsigned chunk_bits = 0u; // the blocks of this chunk
#pragma unroll
            for (int i = 0; i < LCH; i++)
                chunk_bits |= a0 + i < L ? 1u << (L - 1 - (a0 + i)) : 0u;
            const bool any_live = __ballot((livem & chunk_bits) != 0u) != 0ull;
            // exact emission: the accumulator of n = 3 (m = 2 marched segments) takes the arithmetic of the N = 3 plan
            const int i_n3 = exact_emis ? L - 2 - a0 : -1;

            for (int kb = 0; kb < K; kb += VEC) {
                double acc[LCH][VEC]; // emission: the running Iv of every suffix; gain-only: its running gl
                unsigned wnan = 0u;   // emission, bit i * VEC + v: a NaN or infinity among frequency v's lineshape values since suffix i began
#pragma unroll
                for (int i = 0; i < LCH; i++) {
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        acc[i][v] = 0.0;
                }
                // one sub-segment for the first NL accumulators: the walk of rt_step_rscan.hip, its factor taken once
                auto slot_step = [&](auto nl_tag, int s) {
                    constexpr int NL = decltype(nl_tag)::value;
                    asm volatile("" : "+s"(s));
                    const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, flags_steps, backward);
                    const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                    const FVec w     = *reinterpret_cast<const FVec *>(row);
                    if (EMIS) {
                        const float g1 = sl.g, e1 = sl.e;
                        unsigned wn = 0u;
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            wn |= !(fabsf(w.v[v]) <= FLT_MAX) ? 1u << v : 0u;
                        constexpr unsigned spread = NL >= 4 ? 0x1111u : NL == 3 ? 0x111u : NL == 2 ? 0x11u : 0x1u;
                        static_assert(VEC == 4 && LCH <= 4, "wnan keeps VEC bits per accumulator, four accumulators at most");
                        wnan |= wn * spread;
                        if (fabsf(g1) >= RT_RS_MIN && fabsf(g1) <= H.gs_cap && !exact_emis) {
                            const double r1 = div_fast((double) e1, (double) g1);
                            ase_factor(g1, w.v, tab, [&](const int v, const double em1) {
#pragma unroll
                                for (int i = 0; i < NL; i++)
                                    acc[i][v] = fma(em1, acc[i][v] + r1, acc[i][v]);
                            });
                        } else if (g1 != 0.0f || e1 != 0.0f) {
#pragma unroll
                            for (int v = 0; v < VEC; v++) {
                                const AseUpdate u = ase_update_factors(g1, e1, w.v[v], tab);
#pragma unroll
                                for (int i = 0; i < NL; i++)
                                    acc[i][v] = i == i_n3 ? u.apply_n3(acc[i][v]) : u.apply(acc[i][v]);
                            }
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < NL; i++) {
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                acc[i][v] += (double) sl.g * (double) w.v[v];
                        }
                    }
                };
                if (any_live) {
                    // the joining part: segment a0 + I is walked with accumulators 0 .. I
#define LSPEC_JOIN(I)                                                                                            \
    if (I < LCH && a0 + I < L) {                                                                                 \
        _Pragma("unroll 1") for (int t = 0; t < RT_N_SUB; t++)                                                   \
            slot_step(std::integral_constant<int, (I < LCH ? I + 1 : LCH)>{}, (a0 + I) * RT_N_SUB + t);          \
    }
                    LSPEC_JOIN(0)
                    LSPEC_JOIN(1)
                    LSPEC_JOIN(2)
                    LSPEC_JOIN(3)
#undef LSPEC_JOIN
                    // ... and the segments behind the chunk's last start with all of them
#pragma unroll 1
                    for (int s = (a0 + LCH) * RT_N_SUB; s < S; s++)
                        slot_step(std::integral_constant<int, LCH>{}, s);
                }
                // ---- the walk has reached the end of the record: the rows of the chunk ----
#pragma unroll
                for (int i = 0; i < LCH; i++) {
                    if (a0 + i < L) {
                        double Iv[VEC];
                        finish(acc[i], wnan >> (i * VEC), f0[i], kb, Iv);
                        stage_row(i, L - 1 - (a0 + i), Iv, kb);
                    }
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                for (int i = 0; i < LCH && a0 + i < L; i++)
                    flush_row(i, L - 1 - (a0 + i), kb);
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
