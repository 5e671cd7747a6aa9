// rt_spec_tile.inc -- what the tile functions of spectra mode share: spec_tile (rt_spec.hip), spec_seeds_tile
// (rt_spec_seeds.hip) and the two halves of spec_ase_seeds_tile (rt_spec_ase_seeds.hip).  The seed factors of a seed set
// also serve length spectra (rt_spec_scan_seeds.hip, rt_spec_scan_ase_seeds.hip, rt_spec_scan_seeds_walk.inc).
//
// Fragments of a function body (rt_tile_rec.inc says why text and not function templates); parameters are macros that the
// includer defines and undefines around the include.  The includer defines which part it wants.
//   SPEC_TILE_HEAD      the tile head: the constants, the preamble (rt_tile_ray.inc), the exit ray (Helper.h:514-521), the ray2
//                       store, the probe, error -1.  Reads SF, H, hflags, C, tile, lane;
//                         SPEC_TILE_NEED_RAY      TILE_NEED_RAY of rt_tile_ray.inc
//                         SPEC_TILE_RAY2          ray2 [n_rays] of the run
//                         SPEC_TILE_AT_EXIT       (optional) statements of a ray without error -1, behind its exit ray, or
//                         SPEC_TILE_HEAD_FACTORS  (optional) there, unless the ray has escaped, the text of SPEC_TILE_FACTORS
//                                                 with its parameters.  (The seed factors of spec_tile and spec_seeds_tile
//                                                 stay under the test the exit ray stands under: taken under a test of
//                                                 their own behind it, rt_spec_kernel<SF, false> came out with other registers.)
//                         SPEC_TILE_ERR1_CODES    (optional) statements: bit 1 into the code words of the pass
//                       Declares S, K, Kp, n_rays, row0, ridx, have, backward, rrec, rec, probe_on, what rt_tile_ray.inc
//                       declares (m, fl, steps, err1, ray, R, report_failure), and r2.
//   SPEC_TILE_FACTORS   the seed factors of a seed set, place_ray's arithmetic and order (Helper.h:523-533; step_seeds_tile):
//                       rscan_seed_factor on the seed where it lies in the argument block (no copy of a DevSeed: no stack
//                       frame), the seeds in a loop the compiler does not unroll, the factor filed by selects
//                       (rt_step_rscan_seeds.hip).  Its text stands inside that of the head, below: the conditional blocks of
//                       the two are not exclusive.  Reads NS, n_seed, Q->tabs;
//                         SPEC_TILE_FS         the array [NS] the factors go to
//                         SPEC_TILE_POINT      statements that declare px, py, pa, pb (float or double; widened in the call,
//                                              inside the loop): position and angles of the point the seeds are taken at
//                         SPEC_TILE_AT_POINT   (optional) a condition: where it does not hold the launch ray is a point of the
//                                              forward ray grid, and the factor is the product of the seed's tabulated factors
//                                              (RT_SEED_GRID_POINT / RT_SEED_GRID_FACTOR; reads R, ridx).  Without it: no grid.
//   SPEC_TILE_EMISSION  the loop of a row block that leaves as the values the lanes computed: per frequency batch
//                       rt_tile_batch.inc (emission, or gain-only with one seed), the -2 / -3 scan, the staging of 16
//                       frequencies of the 64 rows and their stores as 128-byte row segments, the narrower last group, the
//                       8-byte path of a ragged tile or an odd K (rt_spec.hip says why ordinary stores).  Reads what
//                       rt_tile_batch.inc reads (EMIS, f0, sfk, the decode of rt_tile_rec.inc), live, any_live, wide_ok, stage;
//                         SPEC_TILE_IV   Iv [n_rays][K] of the block
//                       Declares iv_min and has_nan: negative <=> error -2, error -3 unless -2.
//   SPEC_TILE_SEEDS     the gain-only loop of the seeds' row blocks (rt_spec_seeds.hip says what is staged and why), and the
//                       codes per seed behind it.  Reads the decode of rt_tile_rec.inc, Q->tabs.fk, Q->out, n_seed, NS,
//                       live_mask, wide_ok, blk_rows, stage (the factors staged in columns SPEC_SEEDS_F0 ..), err1; ORs into code;
//                         SPEC_TILE_FS          the seed factors of this lane's ray [NS]
//                         SPEC_TILE_LIVE        the lane's ray has rows under a seed, and
//                         SPEC_TILE_ANY_LIVE    some lane's has
//                         SPEC_TILE_GS          the gain sums of the decode, SF > 0 (spec_ase_seeds_tile: an opaque copy)
//                         SPEC_TILE_BLOCK(s)    the row block of seed s
//                         SPEC_TILE_CODE(s)     its code word
#if defined(SPEC_TILE_HEAD)
    const int S           = SF ? SF : H.L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned row0   = tile * WAVE;
    const unsigned ridx   = row0 + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = H.method == 1;
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;

    // ---- per-ray preamble, once: record, -1 test, exit ray (Helper.h:514-521) ----
#define TILE_NEED_RAY SPEC_TILE_NEED_RAY
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    rt_ray r2 = { 0.0f, 0.0f, 0.0f, 0.0f }; // (the reference leaves ray2 untouched on error -1: zeros here)
    if (have && !err1) {
        r2.x = m.px; // Helper.h:518-521
        r2.y = m.py;
        r2.a = atanf_flt32_kernel(m.sx / m.sz) * 1e3f;
        r2.b = atanf_flt32_kernel(m.sy / m.sz) * 1e3f;
#ifdef SPEC_TILE_AT_EXIT
        SPEC_TILE_AT_EXIT
#endif
#ifdef SPEC_TILE_HEAD_FACTORS
        if (!(fl & F_ESCAPED)) { // (closed behind the factors, below)
#endif
#endif // (the head goes on behind the factors: `if (have && !err1)` is still open)
    // ---- SPEC_TILE_FACTORS: a part of its own, or the head's, under the two tests above ----
#if defined(SPEC_TILE_FACTORS) || defined(SPEC_TILE_HEAD_FACTORS)
#ifdef SPEC_TILE_AT_POINT
    if (SPEC_TILE_AT_POINT) {
#else
    {
#endif
        SPEC_TILE_POINT
#pragma unroll 1
        for (int s = 0; s < n_seed; s++) {
            const double f = rscan_seed_factor(&Q->tabs.seed[s], (double) px, (double) py, (double) pa, (double) pb);
#pragma unroll
            for (int t = 0; t < NS; t++)
                SPEC_TILE_FS[t] = t == s ? f : SPEC_TILE_FS[t];
        }
    }
#ifdef SPEC_TILE_AT_POINT
    else {
        // the launch ray is a grid point: product of the seed's tabulated factors (RT_SEED_GRID_FACTOR)
        RT_SEED_GRID_POINT(R, ridx)
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (s < n_seed) {
                const double *sf         = Q->tabs.sf[s];
                const unsigned char *sin = Q->tabs.sin[s];
                RT_SEED_GRID_FACTOR(SPEC_TILE_FS[s], Q->tabs.seed[s].f0, sf, sin)
            }
        }
    }
#endif
#endif
#if defined(SPEC_TILE_HEAD) // ---- the head, second half ----
#ifdef SPEC_TILE_HEAD_FACTORS
        } // (not escaped)
#endif
    } // (have && !err1)
    if (have) {
        SPEC_TILE_RAY2[ridx] = r2;
        if (probe_on) {
            C->probe.ray2[ridx]  = r2;
            C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
            C->probe.steps[ridx] = steps;
        }
    }
    if (err1) { // error -1: reported once, and every code word of the pass has the bit
        report_failure(1u << 1);
#ifdef SPEC_TILE_ERR1_CODES
        SPEC_TILE_ERR1_CODES
#endif
    }
#elif defined(SPEC_TILE_FACTORS) // (above)
#elif defined(SPEC_TILE_EMISSION)
    double iv_min = 0.0;   // min over k of Iv, NaNs ignored: negative <=> error -2
    bool has_nan  = false; // error -3 unless -2 (Helper.h:588-593: negative wins)
    for (int kb = 0; kb < K; kb += VEC) {
        double Iv[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            Iv[j] = 0.0;
        if (any_live) { // (else nothing to integrate: the rows are zeros)
#define TILE_READ_SLOT rec_slot_lazy
#define TILE_REREAD live
#include "rt_tile_batch.inc"
#undef TILE_READ_SLOT
#undef TILE_REREAD
        }
        // ---- scan (Helper.h:582-587) and staging: the lane's four values into its staging row ----
        double *mine = stage + lane * XS_ROW + (kb & 12);
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const double v = (live && kb + j < K) ? Iv[j] : 0.0; // (the padding columns K .. Kp-1 are not part of the spectrum)
            iv_min         = fmin(iv_min, v);
            has_nan        = has_nan || v != v;
            mine[j]        = v;
        }
        if ((kb & 12) == 12 || kb + VEC >= K) {
            __builtin_amdgcn_wave_barrier();
            const int kbase = kb & ~15;
            const int width = K - kbase < 16 ? K - kbase : 16; // frequencies of this group
            if (wide_ok && width == 16) {
                // eight lanes cover the 128 staged bytes of a row, a store instruction eight rows
                double *dst        = SPEC_TILE_IV + ((size_t) (row0 + (unsigned) (lane >> 3)) * (size_t) K + (size_t) (kbase + 2 * (lane & 7)));
                const size_t gstep = (size_t) 8 * (size_t) K; // eight rows on
                const double *src  = stage + (lane >> 3) * XS_ROW + 2 * (lane & 7);
#pragma unroll 4
                for (int g = 0; g < WAVE / 8; g++)
                    SPEC_STORE16(src + g * 8 * XS_ROW, dst + (size_t) g * gstep);
            } else if (wide_ok) {
                // the last, narrower group of a row (2 .. 14 frequencies): still 16 bytes per lane, the wave's lanes dealt over
                // the 64 x hw pieces row by row.  (Folding a left-over of two frequencies into the group before it, as rows
                // of 18 in the two spare doubles of the staging rows, was built and measured: seed_small, K = 82, 2.375
                // against 2.413 ms, the stand-in, which has no such left-over, 1.254 against 1.226 ms.  Not kept.)
                const unsigned hw = (unsigned) width >> 1; // 16-byte pieces per row
                for (unsigned q = (unsigned) lane; q < WAVE * hw; q += WAVE) {
                    const unsigned row = q / hw, piece = q - row * hw;
                    SPEC_STORE16(stage + row * XS_ROW + 2 * piece, SPEC_TILE_IV + ((size_t) (row0 + row) * (size_t) K + (size_t) kbase + 2 * piece));
                }
            } else {
                // ragged tile or odd K: 8 bytes per lane, four rows per instruction
                const int k = kbase + (lane & 15);
#pragma unroll 4
                for (int g = 0; g < WAVE / 4; g++) {
                    const unsigned row = row0 + (unsigned) (4 * g + (lane >> 4));
                    if (row < n_rays && k < K)
                        SPEC_TILE_IV[(size_t) row * (size_t) K + (size_t) k] = stage[(4 * g + (lane >> 4)) * XS_ROW + (lane & 15)];
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
#elif defined(SPEC_TILE_SEEDS)
    double iv_min[NS]; // per seed: min over k of Iv, NaNs ignored: negative <=> error -2
    unsigned nanm = 0u; // bit s: a NaN among the values of seed s: error -3 unless -2
#pragma unroll
    for (int s = 0; s < NS; s++)
        iv_min[s] = 0.0;

    for (int kb = 0; kb < K; kb += VEC) {
        // gain only, Helper.h:569-580: f64 products summed in sub-segment order (the text of rt_tile_batch.inc); once
        double gl[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            gl[j] = 0.0;
        bool with_exp = false;
        if (SPEC_TILE_ANY_LIVE) { // (else nothing to integrate: the rows are zeros)
            if (SF) {
                FVec w[SF ? SF : 1];
                load_rows(w, kb);
#pragma unroll
                for (int s = 0; s < SF; s++) {
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        gl[j] += (double) SPEC_TILE_GS[s] * (double) w[s].v[j];
                }
            } else {
                for (int s = 0; s < S; s++) {
                    const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
                    const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                    const FVec w     = *reinterpret_cast<const FVec *>(row);
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        gl[j] += (double) sl.g * (double) w.v[j];
                }
            }
            // Iv_s = f0_s f_s[4][k] exp(gl); for f0_s = 0 that is exactly 0 unless exp overflows (0 * inf): a wave none of whose
            // lanes needs the exponential under any seed skips it
            bool need = false;
#pragma unroll
            for (int s = 0; s < NS; s++)
                need = need || SPEC_TILE_FS[s] != 0.0;
#pragma unroll
            for (int j = 0; j < VEC; j++)
                need = need || gl[j] > 700.0 || gl[j] != gl[j];
            with_exp = __ballot(need) != 0ull;
        }
        double eg[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            eg[j] = 1.0;
        if (with_exp)
            exp_tab_vec(gl, tab, eg);
        // ---- the exponentials into the lane's staging row; per seed the values of this lane for its scan (Helper.h:582-587) ----
        // (eg = 1 where the wave skipped the exponential: x * 1.0 is x, so the storing lanes need not know)
        double *mine = stage + lane * XS_ROW + (kb & 12);
#pragma unroll
        for (int j = 0; j < VEC; j++)
            mine[j] = eg[j];
        if (SPEC_TILE_ANY_LIVE) {
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const ConstF64 sk = (ConstF64) (unsigned long long) Q->tabs.fk[s];
#pragma unroll
                    for (int j = 0; j < VEC; j++) {
                        const double v = (SPEC_TILE_LIVE && kb + j < K) ? (SPEC_TILE_FS[s] * sk[kb + j]) * eg[j] : 0.0; // (the padding columns K .. Kp-1 are not part of the spectrum)
                        iv_min[s]      = fmin(iv_min[s], v);
                        nanm |= v != v ? 1u << s : 0u;
                    }
                }
            }
        }
        if ((kb & 12) == 12 || kb + VEC >= K) {
            __builtin_amdgcn_wave_barrier();
            const int kbase = kb & ~15;
            const int width = K - kbase < 16 ? K - kbase : 16; // frequencies of this group
            // a value on its way out: (f0_s sfk_s[k]) eg of a live row, +0 of any other (a select: 0 * x would give NaN or -0)
            auto out2 = [&](const double *rowp, const int c, const int s, const bool lv, const f64x2s fk2) {
                const f64x2s e2 = *reinterpret_cast<const f64x2s *>(rowp + c);
                const double fr = rowp[SPEC_SEEDS_F0 + s];
                f64x2s r;
                r.x = lv ? (fr * fk2.x) * e2.x : 0.0;
                r.y = lv ? (fr * fk2.y) * e2.y : 0.0;
                return r;
            };
            if (wide_ok && width == 16) {
                // eight lanes cover the 128 bytes of a row, a store instruction eight rows, as in SPEC_TILE_EMISSION
                const int c = 2 * (lane & 7);
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double *fk = Q->tabs.fk[s] + kbase + c;
                    f64x2s fk2;
                    fk2.x       = fk[0];
                    fk2.y       = fk[1];
                    double *dst = Q->out.Iv + (size_t) (SPEC_TILE_BLOCK(s)) * blk_rows * (size_t) K + ((size_t) (row0 + (unsigned) (lane >> 3)) * (size_t) K + (size_t) (kbase + c));
                    const size_t gstep = (size_t) 8 * (size_t) K; // eight rows on
#pragma unroll 4
                    for (int g = 0; g < WAVE / 8; g++) {
                        const int row      = 8 * g + (lane >> 3);
                        const double *srow = stage + row * XS_ROW;
                        const f64x2s r     = out2(srow, c, s, ((live_mask >> row) & 1ull) != 0ull, fk2);
                        *reinterpret_cast<f64x2s *>(dst + (size_t) g * gstep) = r;
                    }
                }
            } else if (wide_ok) {
                // the last, narrower group of a row (2 .. 14 frequencies): 16 bytes per lane, the lanes dealt over the pieces
                const unsigned hw = (unsigned) width >> 1; // 16-byte pieces per row
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double *fk = Q->tabs.fk[s] + kbase;
                    double *blk      = Q->out.Iv + (size_t) (SPEC_TILE_BLOCK(s)) * blk_rows * (size_t) K;
                    for (unsigned q = (unsigned) lane; q < WAVE * hw; q += WAVE) {
                        const unsigned row = q / hw, piece = q - row * hw;
                        f64x2s fk2;
                        fk2.x          = fk[2 * piece];
                        fk2.y          = fk[2 * piece + 1];
                        const f64x2s r = out2(stage + row * XS_ROW, (int) (2 * piece), s, ((live_mask >> row) & 1ull) != 0ull, fk2);
                        *reinterpret_cast<f64x2s *>(blk + ((size_t) (row0 + row) * (size_t) K + (size_t) kbase + 2 * piece)) = r;
                    }
                }
            } else {
                // ragged tile or odd K: 8 bytes per lane, four rows per instruction
                const int k = kbase + (lane & 15);
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double *fk = Q->tabs.fk[s];
                    double *blk      = Q->out.Iv + (size_t) (SPEC_TILE_BLOCK(s)) * blk_rows * (size_t) K;
                    const double fkk = k < K ? fk[k] : 0.0;
#pragma unroll 4
                    for (int g = 0; g < WAVE / 4; g++) {
                        const int row = 4 * g + (lane >> 4);
                        if (row0 + (unsigned) row < n_rays && k < K) {
                            const double *srow = stage + row * XS_ROW;
                            const bool lv      = ((live_mask >> row) & 1ull) != 0ull;
                            blk[(size_t) (row0 + (unsigned) row) * (size_t) K + (size_t) k] = lv ? (srow[SPEC_SEEDS_F0 + s] * fkk) * srow[lane & 15] : 0.0;
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    // ---- the codes per seed: -1 of the ray, else -2 over -3 (Helper.h:588-593: negative wins); the includer reports a failing
    // ray once, with the OR of its codes ----
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            const bool bad_neg = SPEC_TILE_LIVE && iv_min[s] < 0.0, bad_nan = SPEC_TILE_LIVE && ((nanm >> s) & 1u) != 0u;
            if (have)
                Q->out.err[(size_t) (SPEC_TILE_BLOCK(s)) * blk_rows + ridx] = err1 ? -1 : (bad_neg ? -2 : (bad_nan ? -3 : 0));
            if (bad_neg || bad_nan) {
                const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                code |= c;
                atomicOr(&SPEC_TILE_CODE(s), c);
            }
        }
    }
#else
#error "rt_spec_tile.inc: define SPEC_TILE_HEAD, SPEC_TILE_FACTORS, SPEC_TILE_EMISSION or SPEC_TILE_SEEDS"
#endif
