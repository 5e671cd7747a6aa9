// rt_step_scan_walk.inc -- the forward walk of a chunk of lengths in step mode with a length scan: the loop over the frequency
// batches of step_scan_tile (rt_step_scan.hip), step_scan_seeds_tile (rt_step_scan_seeds.hip) and both halves of
// step_scan_ase_seeds_tile (rt_step_scan_ase_seeds.hip).
//
// Per frequency batch the walk over the slots starts at slot 0: the slots below the chunk (s_lo = 3 j0 of them) are
// integrated again without depositing, then RT_N_SUB slots per length of the chunk.  The arithmetic of a slot is the SF = 0
// text of rt_tile_batch.inc, the choice per slot -- ase_step where the sub-segment is regular, ase_update otherwise and in
// the exact mode, wnan for a NaN or infinity among a frequency's lineshape values (0 * NaN on the CPU); gain-only the f64
// product sum -- so every Iv_j[k] is the double rt_step_kernel<0, EMIS> computes on the prefix problem.  Whenever the walk
// reaches a length (slot 3 j - 1) it finishes Iv_j, updates the sum over k and the sign test of every record of that length
// (min over k of Iv negative, NaNs ignored: error -2, Helper.h:582-594; the sum is RayTraceImageCPU.cpp:66, (2.0 * dv) * Iv)
// and, except in the checking pass of a failing run, adds the E_v wave sum over the lanes that deposit into the record to
// the record's accumulator (rt_step_evsum.inc).
//
// Register notes.  The slot index is made opaque: the slot addresses of a whole chunk, hoisted out of the frequency loop as
// invariants, cost eight registers the loop does not have.  Lengths and seeds are unrolled under wave-uniform tests, so that
// nothing per (record, length) is indexed memory.  (The slot reads m.flags_steps, not the copy that the backward walks take:
// with the copy rt_step_scan_ase_seeds_kernel came out with its register moves in another order.)
//
// A fragment of a function body (rt_tile_rec.inc says why text); the includer defines which walk it wants:
//   SCAN_WALK_EMISSION   acc is the running Iv; one record per length, record 0
//   SCAN_WALK_SEED       gain-only, acc is the running gl; one record per length: Iv = f0 f[4][k] exp(gl), a wave none of whose
//                        lanes needs the exponential skips it (rt_tile_batch.inc).  Reads f0_launch (a double), sfk, seeded
//   SCAN_WALK_SEEDS      gain-only with a seed set: exp(gl) once (needed if any seed's f0 != 0, or gl > 700, or gl is a NaN),
//                        then per seed s < n_seed Iv[v] = (f0_s sfk_s[kb + v]) eg[v] -- the association of the single-seed
//                        walk, so every Iv is the double a plan created with seed s computes.  Reads f0_launch[NS], Z->tabs.fk,
//                        n_seed, NS, seeded;
//                          SCAN_WALK_REC(s)   the record of seed s (s; 1 + s behind an ASE record)
// All read LCH, j0, s_lo, L, S, K, Kp, H, rec, rrec, m.flags_steps, backward, exact_emis, tab, dv2, safe_check, and the E_v sum's
// xpose, lane, lds_ev; with r the record (0 where there is one per length):
//   SCAN_WALK_SUM(r)        the sum over k of record r at length j0 + li + 1, an lvalue (angsum[li], angsum[r][li])
//   SCAN_WALK_DEPOSITS(r)   the lane deposits into record r at that length
//   SCAN_WALK_SCALE(r)      (optional) the scale of record r where it is not H.scale
// Bit r LCH + li of `neg` is set by a negative Iv; record r at length j is accumulator block r L + j - 1 of lds_ev.
for (int kb = 0; kb < K; kb += VEC) {
    double acc[VEC];
#if defined(SCAN_WALK_EMISSION)
    bool wnan[VEC];
#endif
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        acc[v] = 0.0;
#if defined(SCAN_WALK_EMISSION)
        wnan[v] = false;
#endif
    }
    auto slot_step = [&](int s) {
        asm volatile("" : "+s"(s));
        const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
        const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
        const FVec w     = *reinterpret_cast<const FVec *>(row);
#if defined(SCAN_WALK_EMISSION)
        const float g1 = sl.g, e1 = sl.e;
#pragma unroll
        for (int v = 0; v < VEC; v++)
            wnan[v] = wnan[v] || !(fabsf(w.v[v]) <= FLT_MAX);
        if (fabsf(g1) >= RT_RS_MIN && fabsf(g1) <= H.gs_cap && !exact_emis) {
            const double r1 = div_fast((double) e1, (double) g1);
            ase_step(acc, g1, r1, w.v, tab);
        } else if (g1 != 0.0f || e1 != 0.0f) {
#pragma unroll
            for (int v = 0; v < VEC; v++)
                acc[v] = ase_update(acc[v], g1, e1, w.v[v], tab);
        }
#else
#pragma unroll
        for (int v = 0; v < VEC; v++)
            acc[v] += (double) sl.g * (double) w.v[v];
#endif
    };
#pragma unroll 1
    for (int s = 0; s < s_lo; s++)
        slot_step(s);
#pragma unroll
    for (int li = 0; li < LCH; li++) {
        if (j0 + li < L) {
#pragma unroll 1
            for (int t = 0; t < RT_N_SUB; t++)
                slot_step(s_lo + li * RT_N_SUB + t);
            // ---- the walk has reached length j0 + li + 1 ----
#if defined(SCAN_WALK_SEEDS)
            const bool carries = ((seeded >> li) & 1u) != 0u;
            bool need          = false;
#pragma unroll
            for (int s = 0; s < NS; s++)
                need = need || (carries && f0_launch[s] != 0.0);
#pragma unroll
            for (int v = 0; v < VEC; v++)
                need = need || acc[v] > 700.0 || acc[v] != acc[v];
            const bool with_exp = __ballot(need) != 0ull;
            double eg[VEC];
#pragma unroll
            for (int v = 0; v < VEC; v++)
                eg[v] = 1.0;
            if (with_exp)
                exp_tab_vec(acc, tab, eg);
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const int r        = SCAN_WALK_REC(s);
                    const ConstF64 sfk = (ConstF64) (unsigned long long) Z->tabs.fk[s];
                    const double f0    = carries ? f0_launch[s] : 0.0;
                    double Iv[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        Iv[v] = f0 * sfk[kb + v];
                    if (with_exp) {
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] *= eg[v];
                    }
#else
            {
                {
                    enum { r = 0 };
                    double Iv[VEC];
#if defined(SCAN_WALK_EMISSION)
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        Iv[v] = wnan[v] ? __builtin_nan("") : acc[v];
#else
                    const double f0 = ((seeded >> li) & 1u) ? f0_launch : 0.0;
                    bool need       = f0 != 0.0;
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
#endif
#endif
                    // (either way: Iv of record r at this length)
#pragma unroll
                    for (int v = 0; v < VEC; v++) {
                        neg |= Iv[v] < 0.0 ? 1u << (r * LCH + li) : 0u;
                        SCAN_WALK_SUM(r) += dv2[kb + v] * Iv[v];
                    }
                    if (!safe_check) {
                        const bool dep = SCAN_WALK_DEPOSITS(r);
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX (r * L + j0 + li) * Kp + kb
#ifdef SCAN_WALK_SCALE
                        const double scale_r = SCAN_WALK_SCALE(r);
#define EV_SUM_SCALE scale_r
#endif
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
#ifdef SCAN_WALK_SCALE
#undef EV_SUM_SCALE
#endif
                    }
                }
            }
        }
    }
}
