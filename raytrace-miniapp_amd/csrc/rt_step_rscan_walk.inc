// rt_step_rscan_walk.inc -- the backward walk of a chunk of suffixes in step mode with a suffix scan: the loop over the
// frequency batches of step_rscan_tile (rt_step_rscan.hip), step_rscan_seeds_tile (rt_step_rscan_seeds.hip) and both halves of
// step_rscan_ase_seeds_tile (rt_step_rscan_ase_seeds.hip).
//
// The recurrence of a suffix starts with Iv = 0 at its own first slot, so the suffixes do not share a running value as the
// prefixes do -- but in emission mode they share everything of a slot that is expensive: e^gl - 1 and rs depend on the slot
// alone (ase_step, rt_freq.hip), the update is Iv = fma(em1, Iv + rs, Iv), one add and one fma per accumulator.  A chunk
// is LCH start segments a0 .. a0 + LCH - 1 (start segment a is record n = N - a, block L - 1 - a): per frequency batch ONE
// walk over slots 3 a0 .. S - 1 with LCH accumulators of VEC doubles in registers, accumulator i joining at slot 3 (a0 + i).
// The joining part is unrolled so that the number of live accumulators is a compile-time count (a loop variable is no
// template argument, hence the four statements of RSCAN_JOIN); no slot is integrated twice inside a chunk.  Every Iv_n[k] is
// the double rt_step_kernel<0, EMIS> computes on the suffix problem: ase_factor is ase_step up to its last line, irregular
// sub-segments and the exact mode take ase_update per accumulator, the gain-only mode the same f64 product sum and one
// ballot-skipped exp_tab_vec per record.  At the end of the record the walk finishes Iv of every suffix of the chunk, updates
// the sum over k and the sign test of its records (error -2, Helper.h:582-594; RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv) and,
// except in the checking pass of a failing run, adds the E_v wave sum to the record's accumulator (rt_step_evsum.inc).
//
// Register notes.  The slot index is opaque, as in rt_step_scan_walk.inc: no slot addresses hoisted out of the frequency
// loop.  The rare update goes through ase_update_call: inlined NL * VEC times into each of the five copies of the slot text
// the rare path set the register count -- 128 VGPRs and 68 spilled at four accumulators, 118 and none with the call.
//
// A fragment of a function body (rt_tile_rec.inc says why text); the includer defines which walk it wants:
//   RSCAN_WALK_EMISSION   acc[i] is the running Iv of suffix i, wnan bit i * VEC + v a NaN or infinity among frequency v's
//                         lineshape values since suffix i began; one record per suffix, record 0
//   RSCAN_WALK_SEED       gain-only, acc[i] the running gl; one record per suffix: Iv = f0[i] f[4][k] exp(gl).  Reads f0[LCH], sfk
//   RSCAN_WALK_SEEDS      gain-only with a seed set: exp(gl) once per suffix, then Iv per seed s < n_seed.  Reads f0[NS][LCH],
//                         Z->tabs.fk, n_seed, NS;
//                           RSCAN_WALK_REC(s)   the record of seed s (s; 1 + s behind an ASE record)
// All read LCH, a0, L, S, K, Kp, H, rec, rrec, flags_steps, backward, exact_emis, tab, dv2, safe_check, has_pix, live, and the
// E_v sum's xpose, lane, lds_ev; with s the seed (0 where there is one record per suffix):
//   RSCAN_WALK_SUM(s)     the sum over k of seed s under suffix i, an lvalue (angsum[i], angsum[s][i])
//   RSCAN_WALK_SCALE(s)   (optional) the scale of the record where it is not H.scale
// Bit s LCH + i of `live`: the ray is live under that record; of `neg`: set by a negative Iv.
for (int kb = 0; kb < K; kb += VEC) {
    double acc[LCH][VEC];
#if defined(RSCAN_WALK_EMISSION)
    unsigned wnan = 0u;
#endif
#pragma unroll
    for (int i = 0; i < LCH; i++) {
#pragma unroll
        for (int v = 0; v < VEC; v++)
            acc[i][v] = 0.0;
    }
    // one sub-segment for the first NL accumulators: the SF = 0 text of rt_tile_batch.inc, its factor taken once
    auto slot_step = [&](auto nl_tag, int s) {
        constexpr int NL = decltype(nl_tag)::value;
        asm volatile("" : "+s"(s));
        const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, flags_steps, backward);
        const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
        const FVec w     = *reinterpret_cast<const FVec *>(row);
#if defined(RSCAN_WALK_EMISSION)
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
            for (int i = 0; i < NL; i++) {
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[i][v] = ase_update_call(acc[i][v], g1, e1, w.v[v], tab);
            }
        }
#else
#pragma unroll
        for (int i = 0; i < NL; i++) {
#pragma unroll
            for (int v = 0; v < VEC; v++)
                acc[i][v] += (double) sl.g * (double) w.v[v];
        }
#endif
    };
    // the joining part: segment a0 + I is walked with accumulators 0 .. I
#define RSCAN_JOIN(I)                                                                                            \
    if (I < LCH && a0 + I < L) {                                                                                 \
        _Pragma("unroll 1") for (int t = 0; t < RT_N_SUB; t++)                                                   \
            slot_step(std::integral_constant<int, (I < LCH ? I + 1 : LCH)>{}, (a0 + I) * RT_N_SUB + t);          \
    }
    RSCAN_JOIN(0)
    RSCAN_JOIN(1)
    RSCAN_JOIN(2)
    RSCAN_JOIN(3)
#undef RSCAN_JOIN
    // ... and the segments behind the chunk's last start with all of them
#pragma unroll 1
    for (int s = (a0 + LCH) * RT_N_SUB; s < S; s++)
        slot_step(std::integral_constant<int, LCH>{}, s);

    // ---- the walk has reached the end of the record: Iv of every suffix of the chunk ----
#pragma unroll
    for (int i = 0; i < LCH; i++) {
        if (a0 + i < L) {
#if defined(RSCAN_WALK_SEEDS)
            bool need = false;
#pragma unroll
            for (int s = 0; s < NS; s++)
                need = need || f0[s][i] != 0.0;
#pragma unroll
            for (int v = 0; v < VEC; v++)
                need = need || acc[i][v] > 700.0 || acc[i][v] != acc[i][v];
            const bool with_exp = __ballot(need) != 0ull;
            double eg[VEC];
#pragma unroll
            for (int v = 0; v < VEC; v++)
                eg[v] = 1.0;
            if (with_exp)
                exp_tab_vec(acc[i], tab, eg);
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
#define RSCAN_WALK_BIT (s * LCH + i)
#define RSCAN_WALK_BLOCK (RSCAN_WALK_REC(s) * L + L - 1 - (a0 + i))
#define RSCAN_WALK_SEED_NO s
                    const ConstF64 sfk = (ConstF64) (unsigned long long) Z->tabs.fk[s];
                    double Iv[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        Iv[v] = f0[s][i] * sfk[kb + v];
                    if (with_exp) {
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] *= eg[v];
                    }
#else
#define RSCAN_WALK_BIT i
#define RSCAN_WALK_BLOCK (L - 1 - (a0 + i))
#define RSCAN_WALK_SEED_NO 0
            {
                {
                    double Iv[VEC];
#if defined(RSCAN_WALK_EMISSION)
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        Iv[v] = ((wnan >> (i * VEC + v)) & 1u) ? __builtin_nan("") : acc[i][v];
#else
                    bool need = f0[i] != 0.0;
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        need = need || acc[i][v] > 700.0 || acc[i][v] != acc[i][v];
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        Iv[v] = f0[i] * sfk[kb + v];
                    if (__ballot(need) != 0ull) {
                        double eg[VEC];
                        exp_tab_vec(acc[i], tab, eg);
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] *= eg[v];
                    }
#endif
#endif
                    // (either way: Iv of seed s, record r, under suffix i)
#pragma unroll
                    for (int v = 0; v < VEC; v++) {
                        neg |= Iv[v] < 0.0 ? 1u << RSCAN_WALK_BIT : 0u;
                        RSCAN_WALK_SUM(RSCAN_WALK_SEED_NO) += dv2[kb + v] * Iv[v];
                    }
                    if (!safe_check) {
                        const bool dep = has_pix && ((live >> RSCAN_WALK_BIT) & 1u) != 0u;
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX RSCAN_WALK_BLOCK * Kp + kb
#ifdef RSCAN_WALK_SCALE
                        const double scale_s = RSCAN_WALK_SCALE(RSCAN_WALK_SEED_NO);
#define EV_SUM_SCALE scale_s
#endif
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
#ifdef RSCAN_WALK_SCALE
#undef EV_SUM_SCALE
#endif
                    }
                }
            }
        }
    }
}
#undef RSCAN_WALK_BIT
#undef RSCAN_WALK_BLOCK
#undef RSCAN_WALK_SEED_NO
