// rt_spec_scan_seeds_walk.inc -- the walk of length spectra with seeds over the march record and its stores: everything of
// spec_scan_seeds_tile (rt_spec_scan_seeds.hip) behind the per-block state, as text, so that the seed half of
// rt_spec_scan_ase_seeds.hip takes the same statements (rt_tile_rec.inc says why text and not a function template).
//
// Two parts; the includer defines which one it wants.
//   SSS_WALK_F0     the seed factors at the launch ray (forward), the text of spectra mode (rt_spec_tile.inc, SPEC_TILE_FACTORS).
//                   Reads NS, n_seed, BACKWARD, have, ridx, R, ray, Q->tabs; declares f0_launch[NS].
//                     SSS_GRID_TABS   the seeds' factor tables on the forward ray grid serve this run (a pointer or a bool)
//   SSS_WALK_TILE   the walk.  Reads BACKWARD, SF (= 0), LCH (= SSS_LCH), NS; H, Q (Q->tabs), n_seed, tab, stage, lane, L, S, K,
//                   Kp, n_rays, row0, rec, rrec, flags_steps, backward, f0_launch[], blk_rays; the bits livem and seedm, which
//                   open_block(mseg, fs) sets and whose seed factors (backward) it leaves in fs[]; adds to negm[] and nanm[];
//                     SSS_OUT_IV   block (0, 0) of the seeds: block jb of seed s is SSS_OUT_IV + (s L + jb) n_rays K
#if defined(SSS_WALK_F0)
    // the seed factors at the launch ray (forward, Helper.h:530-533), in place_ray's own arithmetic as rt_step_scan_seeds.hip takes them
    double f0_launch[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        f0_launch[s] = 0.0;
    if (!BACKWARD && have) {
        // (the loop over the seeds and the product on a ray grid: the text of spectra mode, rt_spec_tile.inc)
#define SPEC_TILE_FACTORS
#define SPEC_TILE_FS f0_launch
#define SPEC_TILE_AT_POINT !(SSS_GRID_TABS)
#define SPEC_TILE_POINT                                                                                                        \
    rt_ray launch = ray;                                                                                                       \
    float ta, tb;                                                                                                              \
    load_ray(R, ridx, launch, ta, tb, false);                                                                                  \
    const double px = (double) launch.x, py = (double) launch.y, pa = (double) launch.a, pb = (double) launch.b;
#include "rt_spec_tile.inc"
#undef SPEC_TILE_POINT
#undef SPEC_TILE_AT_POINT
#undef SPEC_TILE_FS
#undef SPEC_TILE_FACTORS
    }
#elif defined(SSS_WALK_TILE)
    // a full tile and an even K: the pieces of a row leave as 16-byte stores
    const bool wide_ok = row0 + WAVE <= n_rays && (K & 1) == 0;
    // column `col` of the 64 staging rows to block jb of seed s, frequencies kb .. kb + VEC - 1 (rt_spec_scan_tile.inc)
    auto flush_row = [&](const int col, const int s, const int jb, const int kb) {
        double *blk = SSS_OUT_IV + ((size_t) s * (size_t) L + (size_t) jb) * blk_rays * (size_t) K;
#define SPEC_SCAN_FLUSH
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_FLUSH
    };
    // The rows of block jb under every seed from the running gl of the block: exp(gl) once for all seeds, skipped by a wave
    // that has no use for it; then per seed Iv = (f0_s f_s[4][k]) eg, the -2 / -3 scan (Helper.h:582-587) and the lane's VEC
    // values into columns li * NS + s of its staging row
    auto finish_rows = [&](const int li, const int jb, const double (&acc)[VEC], const double (&fs)[NS], const int kb) {
        const bool lv = ((livem >> jb) & 1u) != 0u;
        bool need     = false;
#pragma unroll
        for (int s = 0; s < NS; s++)
            need = need || fs[s] != 0.0;
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
                const ConstF64 sfk = (ConstF64) (unsigned long long) Q->tabs.fk[s];
                double *mine       = stage + lane * XS_ROW + (li * NS + s) * VEC;
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    double x = fs[s] * sfk[kb + v];
                    if (with_exp)
                        x *= eg[v];
                    x = (lv && kb + v < K) ? x : 0.0; // (the padding columns K .. Kp-1 are not part of the spectrum)
                    negm[s] |= x < 0.0 ? 1u << jb : 0u;
                    nanm[s] |= x != x ? 1u << jb : 0u;
                    mine[v] = x;
                }
            }
        }
    };

    if (!BACKWARD) {
        // ---- forward: every block's state first, then one walk per frequency batch ----
#pragma unroll 1
        for (int j = 1; j <= L; j++) {
            double unused[NS];
            open_block(j, unused);
            (void) unused;
        }
        const bool any_live = __ballot(livem != 0u) != 0ull; // (else nothing to integrate: the rows are zeros)
        for (int kb = 0; kb < K; kb += VEC) {
            double acc[VEC]; // the running gl
#pragma unroll
            for (int v = 0; v < VEC; v++)
                acc[v] = 0.0;
#pragma unroll 1
            for (int j = 0; j < L; j++) {
                if (any_live) {
#pragma unroll 1
                    for (int t = 0; t < RT_N_SUB; t++) {
                        // one sub-segment: the gain-only SF = 0 text of rt_tile_batch.inc
                        int s = j * RT_N_SUB + t;
                        asm volatile("" : "+s"(s));
                        const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, flags_steps, backward);
                        const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                        const FVec w     = *reinterpret_cast<const FVec *>(row);
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            acc[v] += (double) sl.g * (double) w.v[v];
                    }
                }
                // ---- the walk has reached length j + 1: row block j of every seed ----
                double fs[NS];
#pragma unroll
                for (int s = 0; s < NS; s++)
                    fs[s] = ((seedm >> j) & 1u) ? f0_launch[s] : 0.0;
                finish_rows(j & (LCH - 1), j, acc, fs, kb);
                if ((j & (LCH - 1)) == LCH - 1 || j == L - 1) {
                    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                    for (int jj = j & ~(LCH - 1); jj <= j; jj++) {
#pragma unroll 1
                        for (int s = 0; s < n_seed; s++)
                            flush_row((jj & (LCH - 1)) * NS + s, s, jj, kb);
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
    } else {
        // ---- backward: the suffixes in chunks of LCH start segments a0 .. a0 + LCH - 1 (start segment a is block L - 1 - a) ----
        for (int a0 = 0; a0 < L; a0 += LCH) {
            double f0[LCH][NS];
#pragma unroll
            for (int i = 0; i < LCH; i++) {
#pragma unroll
                for (int s = 0; s < NS; s++)
                    f0[i][s] = 0.0;
                if (a0 + i < L)
                    open_block(L - (a0 + i), f0[i]);
                // (one state after the other, as rt_step_rscan.hip takes them)
                asm volatile("" ::: "memory");
            }
            unsigned chunk_bits = 0u; // the blocks of this chunk
#pragma unroll
            for (int i = 0; i < LCH; i++)
                chunk_bits |= a0 + i < L ? 1u << (L - 1 - (a0 + i)) : 0u;
            const bool any_live = __ballot((livem & chunk_bits) != 0u) != 0ull;

            for (int kb = 0; kb < K; kb += VEC) {
                double acc[LCH][VEC]; // the running gl of every suffix
#pragma unroll
                for (int i = 0; i < LCH; i++) {
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        acc[i][v] = 0.0;
                }
                // one sub-segment for the first NL accumulators: the walk of rt_step_rscan.hip
                auto slot_step = [&](auto nl_tag, int s) {
                    constexpr int NL = decltype(nl_tag)::value;
                    asm volatile("" : "+s"(s));
                    const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, flags_steps, backward);
                    const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                    const FVec w     = *reinterpret_cast<const FVec *>(row);
#pragma unroll
                    for (int i = 0; i < NL; i++) {
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            acc[i][v] += (double) sl.g * (double) w.v[v];
                    }
                };
                if (any_live) {
                    // the joining part: segment a0 + I is walked with accumulators 0 .. I
#define SSS_JOIN(I)                                                                                              \
    if (I < LCH && a0 + I < L) {                                                                                 \
        _Pragma("unroll 1") for (int t = 0; t < RT_N_SUB; t++)                                                   \
            slot_step(std::integral_constant<int, (I < LCH ? I + 1 : LCH)>{}, (a0 + I) * RT_N_SUB + t);          \
    }
                    SSS_JOIN(0)
                    SSS_JOIN(1)
#undef SSS_JOIN
                    // ... and the segments behind the chunk's last start with all of them
#pragma unroll 1
                    for (int s = (a0 + LCH) * RT_N_SUB; s < S; s++)
                        slot_step(std::integral_constant<int, LCH>{}, s);
                }
                // ---- the walk has reached the end of the record: the rows of the chunk, every seed ----
#pragma unroll
                for (int i = 0; i < LCH; i++) {
                    if (a0 + i < L)
                        finish_rows(i, L - 1 - (a0 + i), acc[i], f0[i], kb);
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                for (int i = 0; i < LCH && a0 + i < L; i++) {
#pragma unroll 1
                    for (int s = 0; s < n_seed; s++)
                        flush_row(i * NS + s, s, L - 1 - (a0 + i), kb);
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
#endif
