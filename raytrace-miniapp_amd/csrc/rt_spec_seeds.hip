#pragma once
// rt_spec_seeds.hip -- spectra mode with the seeds of rt_hip_plan_set_spectra_seeds: RayTrace::calc_ray for every ray of a
// run under up to RT_N_SEED_MAX seed beams, from ONE march and ONE walk over the march record.
//
// The premise is that of rt_step_seeds.hip: neither the march record nor the exit ray holds anything of the seed, which
// enters as Iv_s[k] = (f0_s f_s[4][k]) exp(gl[k]) only (Helper.h:523-533, 569-580).  rt_spec_seeds_kernel<SF> stands where
// rt_spec_kernel<SF, false> stands, gain-only, and has its shell, its LDS and its launch bounds.  Per tile, once: the
// preamble (rt_tile_ray.inc), the -1 test, the exit ray, the record decode (rt_tile_rec.inc, the slots of a lane without a
// live ray zeroed as spec_tile zeroes them).  Per seed: f0_s, in the order of step_seeds_tile -- forward at the launch ray (on
// a ray grid the product of the seed's tabulated factors, RT_SEED_GRID_FACTOR), backward at the exit state; the factor is
// rscan_seed_factor on the seed where it lies in the argument block (no copy of a DevSeed: no stack frame).  Per frequency
// batch: gl[] and exp_tab_vec once -- needed if any seed's f0 != 0, or gl > 700, or gl is a NaN, the rule of
// rt_tile_batch.inc with `need` taken over all seeds as rt_step_seeds.hip argues -- then per seed
// Iv_s[j] = (f0_s sfk_s[kb + j]) eg[j], the double rt_spec_kernel computes on a plan created with seed s, in its
// association; the lane's -2 / -3 scan per seed (Helper.h:582-593: a negative value wins over a NaN).
//
// Outputs, seed-major: Iv [n_seed][n_rays][K] (row stride K), err [n_seed][n_rays], ray2 [n_rays] (error -1 and the exit ray
// do not depend on the seed).  Block 0 is seed 0: the plain accessors of spectra mode serve it.  Every element is written.
//
// The stores.  One [64][XS_ROW] staging per wave fills the CU at 16 waves, so a second one does not fit, and a row cut between
// the seeds leaves as 64-byte pieces (measured: the pass then takes 1.27 .. 1.45 x the two single-seed passes).
// So what is staged is what the seeds share: the wave stages the 16 EXPONENTIALS of a group of its 64 rows, as rt_spec.hip
// stages 16 values, and f0_s of a row once per tile in the two spare doubles of the row.  The storing lanes -- eight per row,
// 16 bytes each, eight rows per instruction, the 128-byte segments of rt_spec.hip -- form (f0_s sfk_s[k]) eg per seed on the way
// out: the same association, so the same doubles as the row's own lane computes for its -2 / -3 scan.  A row that is not live
// leaves as +0 by a select on the wave's live mask (0 * x would give NaN or -0 for some eg and sfk); where the wave skipped the
// exponential eg = 1 is staged, and x * 1 is x.  A last group of 2 .. 14 frequencies leaves as 16-byte pieces dealt over the
// lanes, ragged last tiles and odd K as 8 bytes per lane, as in rt_spec.hip.  No slot is read twice for the stores' sake; the
// two products of a value are formed twice (by the row's lane for the scan, by the storing lane for the store).
//
// Failures: a ray is reported once (rt_tile_ray.inc, report_failure) with the OR of its codes over the seeds;
// DevCtl::seed_code[s] carries the code of seed s, as for a seed set.  Nothing is deposited: no checking repeat.
#include "rt_spec.hip"
#include "rt_step_seeds.hip"
#include "rt_step_rscan.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_spec.hip: the same contractions, the same doubles)

constexpr int SPEC_SEEDS_F0 = 16; // column of f0_0 in a staging row: behind the 16 exponentials of a group
static_assert(SPEC_SEEDS_F0 + RT_N_SEED_MAX <= XS_ROW, "the spare doubles of a staging row hold the seed factors of its ray");

// what rt_spec_seeds_kernel reads beside the frequency kernel's block (through the constant address space, as the cold half)
struct SpecSeedsArg {
    int n_seed;
    int pad;
    SpecOut out; // Iv [n_seed][n_rays][K], ray2 [n_rays], err [n_seed][n_rays]
    SeedTabs tabs;
};
struct SpecSeedsKArg {
    FreqHot hot;
    FreqCold cold;
    SpecSeedsArg set;
};
typedef const RT_CONST_AS SpecSeedsArg *SpecSeedsPtr;

template <int SF>
__device__ __forceinline__ void spec_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SpecSeedsPtr Q, const int n_seed, const double *tab,
                                                double *stage, const unsigned tile, const int lane)
{
    constexpr int NS      = RT_N_SEED_MAX;
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
#define TILE_NEED_RAY (!backward) // the forward seed factors are taken at the launch ray
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    rt_ray r2 = { 0.0f, 0.0f, 0.0f, 0.0f }; // (the reference leaves ray2 untouched on error -1: zeros here)
    double f0[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        f0[s] = 0.0;
    if (have && !err1) {
        r2.x = m.px; // Helper.h:518-521
        r2.y = m.py;
        r2.a = atanf_flt32_kernel(m.sx / m.sz) * 1e3f;
        r2.b = atanf_flt32_kernel(m.sy / m.sz) * 1e3f;
        // ---- per seed: the seed factor, place_ray's arithmetic and order (Helper.h:523-533; step_seeds_tile) ----
        if (!(fl & F_ESCAPED)) {
            if (backward || !R.sf) {
                const double px = backward ? (double) m.px : (double) ray.x, py = backward ? (double) m.py : (double) ray.y;
                const double pa = backward ? (double) r2.a : (double) ray.a, pb = backward ? (double) r2.b : (double) ray.b;
                // (the seeds in a loop the compiler does not unroll, the factor filed by selects -- rt_step_rscan_seeds.hip)
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double f = rscan_seed_factor(&Q->tabs.seed[s], px, py, pa, pb);
#pragma unroll
                    for (int t = 0; t < NS; t++)
                        f0[t] = t == s ? f : f0[t];
                }
            } else {
                // the launch ray is a grid point: product of the seed's tabulated factors (RT_SEED_GRID_FACTOR)
                RT_SEED_GRID_POINT(R, ridx)
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
                        const double *sf         = Q->tabs.sf[s];
                        const unsigned char *sin = Q->tabs.sin[s];
                        RT_SEED_GRID_FACTOR(f0[s], Q->tabs.seed[s].f0, sf, sin)
                    }
                }
            }
        }
    }
    if (have) {
        Q->out.ray2[ridx] = r2;
        if (probe_on) {
            C->probe.ray2[ridx]  = r2;
            C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
            C->probe.steps[ridx] = steps;
        }
    }
    if (err1) { // error -1: reported once, and every seed's code has the bit
        report_failure(1u << 1);
#pragma unroll
        for (int s = 0; s < NS; s++)
            if (s < n_seed)
                atomicOr(&H.ctl->seed_code[s], 1u << 1);
    }
    // a ray with error -1, and one whose every update is the identity (F_SKIP), gets a row of zeros under every seed
    const bool live     = have && !err1 && !(fl & F_SKIP);
    const bool any_live = __ballot(live) != 0ull;

    // ---- the march record of this lane's ray, the slots of a lane without a live ray zeroed (as spec_tile) ----
#define TILE_MASK live
#include "rt_tile_rec.inc"
#undef TILE_MASK
    (void) rs;
    (void) all_small;
    (void) all_regular;
    (void) gv_nan;
    (void) exact_emis;

    // what the storing lanes need of a row beside its exponentials: whether it is live, and its seed factors -- once per tile
    // (the flush of the tile before ended behind a wave barrier; the first flush of this one begins behind one)
    const unsigned long long live_mask = __ballot(live);
#pragma unroll
    for (int s = 0; s < NS; s++)
        stage[lane * XS_ROW + SPEC_SEEDS_F0 + s] = f0[s];

    double iv_min[NS]; // per seed: min over k of Iv, NaNs ignored: negative <=> error -2
    unsigned nanm = 0u; // bit s: a NaN among the values of seed s: error -3 unless -2
#pragma unroll
    for (int s = 0; s < NS; s++)
        iv_min[s] = 0.0;
    // a full tile and an even K: every group that lies inside K leaves as 16-byte stores
    const bool wide_ok    = row0 + WAVE <= n_rays && (K & 1) == 0;
    const size_t blk_rows = (size_t) n_rays; // rows of one seed's block

    for (int kb = 0; kb < K; kb += VEC) {
        // gain only, Helper.h:569-580: f64 products summed in sub-segment order (the text of rt_tile_batch.inc); once
        double gl[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            gl[j] = 0.0;
        bool with_exp = false;
        if (any_live) { // (else nothing to integrate: the rows are zeros)
            if (SF) {
                FVec w[SF ? SF : 1];
                load_rows(w, kb);
#pragma unroll
                for (int s = 0; s < SF; s++) {
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        gl[j] += (double) gs[s] * (double) w[s].v[j];
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
                need = need || f0[s] != 0.0;
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
        if (any_live) {
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const ConstF64 sfk = (ConstF64) (unsigned long long) Q->tabs.fk[s];
#pragma unroll
                    for (int j = 0; j < VEC; j++) {
                        const double v = (live && kb + j < K) ? (f0[s] * sfk[kb + j]) * eg[j] : 0.0; // (the padding columns K .. Kp-1 are not part of the spectrum)
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
                // eight lanes cover the 128 bytes of a row, a store instruction eight rows, as in rt_spec.hip
                const int c = 2 * (lane & 7);
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double *fk = Q->tabs.fk[s] + kbase + c;
                    f64x2s fk2;
                    fk2.x       = fk[0];
                    fk2.y       = fk[1];
                    double *dst = Q->out.Iv + (size_t) s * blk_rows * (size_t) K + ((size_t) (row0 + (unsigned) (lane >> 3)) * (size_t) K + (size_t) (kbase + c));
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
                    double *blk      = Q->out.Iv + (size_t) s * blk_rows * (size_t) K;
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
                    double *blk      = Q->out.Iv + (size_t) s * blk_rows * (size_t) K;
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
    // ---- the codes per seed: -1 of the ray, else -2 over -3; a failing ray is reported once ----
    unsigned code = 0u;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            const bool bad_neg = live && iv_min[s] < 0.0, bad_nan = live && ((nanm >> s) & 1u) != 0u;
            if (have)
                Q->out.err[(size_t) s * blk_rows + ridx] = err1 ? -1 : (bad_neg ? -2 : (bad_nan ? -3 : 0));
            if (bad_neg || bad_nan) {
                const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                code |= c;
                atomicOr(&H.ctl->seed_code[s], c);
            }
        }
    }
    if (code)
        report_failure(code);
}

// The shell of rt_spec_kernel: one work-group of FREQ_WG_WAVES waves per CU, tiles from the eight sharded counters, one
// tile per fetch; LDS, all dynamic: the two exponent tables, then [64][XS_ROW] staging doubles per wave.
template <int SF>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_spec_seeds_kernel(const SpecSeedsKArg A)
{
    const int n_seed = A.set.n_seed;
    // per tile: the cold half and the seeds of the argument block, the flag word and the lane number opaque
#define SPEC_WG_KERNEL
#define SPEC_WG_TILE                                                                                                    \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecSeedsKArg, cold)); \
    SpecSeedsPtr Q = (SpecSeedsPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecSeedsKArg, set)); \
    asm volatile("" : "+s"(C), "+s"(Q)); \
    unsigned hflags = H.flags; \
    int lane_t      = lane; \
    asm volatile("" : "+s"(hflags), "+v"(lane_t)); \
    spec_seeds_tile<SF>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_TILE
#undef SPEC_WG_KERNEL
}

} // namespace rt
