#pragma once
// rt_step_ase_seeds.hip -- step mode of an emission plan that carries ASE seeds (rt_hip_plan_set_ase_seeds): the whole
// per-step record of the application from ONE march.
//
// intensity_step_struct (src/RayTraceStructures.h:361-369) is one buffer: the ASE triple E_v | image | E_ang and one seeded
// triple per seed beam, s < N_seed <= N_SEED_MAX = 2.  The trajectory of RayTrace_calc_ray, its gvl and ivl, the exit
// state, the escape flag and the step count do not depend on use_emis; only evl does (Helper.h:486-489, 502).  The march
// record of an emission plan therefore holds everything the gain-only pass of a seeded run of the same problem reads, and
// rt_step_ase_seeds_kernel leaves 1 + n_seed records from it:
//   record 0       what rt_step_kernel<SF, true> leaves on this plan: the emission recurrence, the text of rt_tile_batch.inc
//                  (tile-wide choice, exact emission and gv_nan included), the plan's scale
//   record 1 + s   what a step run leaves of the same problem created with seed s (use_emis = E0 != NULL && seed == NULL:
//                  E0 present but unused): gain-only, Iv[k] = f0_s f_s[4][k] exp(gl[k]), scale scales[s]
// It stands where rt_step_kernel stands and has the shell of every step pass (rt_step_wg.inc, rt_step_handout.inc: one
// 16-wave work-group per CU, lanes = rays) with n_rec = 1 + n_seed histograms and E_v accumulators.  Per tile, once: the
// preamble (rt_tile_ray.inc), place_ray without its seed half, per seed f0_s as step_seeds_tile computes it (on a forward
// ray grid the product of the seed's tabulated factors, otherwise seed_factor at the launch ray -- method 2 -- or the exit
// ray -- method 1), the record decode (rt_tile_rec.inc).  Per frequency batch the lineshape rows feed the emission
// recurrence and the f64 product sum gl[] with one exp_tab_vec for all seeds, in the association of rt_tile_batch.inc /
// rt_step_seeds.hip: every Iv is the double the plain emission plan, respectively the plain single-seed plan, computes.
// Generic S (<0>): ONE loop over kb, the rows loaded once, row by row inside the emission loop (its slot hook
// TILE_BATCH_SLOT sums gl[]).  SF = 6: the combined loop does not fit the budget of rt_step_kernel<6, true> -- 128 VGPRs
// with 18 spilled and 64 bytes of scratch, where the recurrence alone takes 116 and the seed half alone 102 -- so the seed
// half runs as a SECOND loop over kb in the same tile (HALVES below), which reads the rows again, from the caches: 121
// VGPRs, no scratch, four waves per SIMD (profiles/ase_seeds_kernel_resources.txt).
// Then the E_v wave sum per record (rt_step_evsum.inc, the record's scale); at tile end, per record, the I_ang add and the
// segmented nf scan over the runs of equal pixel, found once.  nf is added by atomics only (no exclusive store).
//
// F_SKIP: the emission march marks a ray whose every gvl / evl sum is zero.  It adds exactly +0 to record 0, but under a
// seed it carries f0_s f_s[4][k] exp(0): F_SKIP masks record 0 only -- there the ray is out of the live mask as in
// rt_step_kernel (a tile none of whose rays is live for record 0 skips the recurrence, as rt_step_kernel returns) --, for the
// seed records it is live.  An escaped ray has seed factor 0 and stays live for record 0.
//
// Failures follow the reference run once per record (rt_step_seeds.hip has them per seed): error -1 puts the ray in no
// record and sets the bit in every record's code; error -2 / -3 under record r removes the ray from record r only.  A
// failing ray is reported once, with the OR of its codes; DevCtl::rec_code[r] holds the code of record r; bad[] gets one bit
// per record, written by the lane that holds the ray; the checking repeat keeps its two passes.
#include "rt_step_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

// what rt_step_ase_seeds_kernel reads beside the frequency kernel's block (through the constant address space, as SeedSetArg)
struct AseSeedsArg {
    int n_seed;
    int pad;
    SeedRec out[1 + RT_N_SEED_MAX];          // record 0: ASE; record 1 + s: seed s
    double scale[1 + RT_N_SEED_MAX];         // of every record (scale[0] is the plan's, FreqHot::scale)
    SeedTabs tabs;
};
static_assert(offsetof(AseSeedsArg, tabs) == 8 + (sizeof(SeedRec) + sizeof(double)) * (1 + RT_N_SEED_MAX) &&
                  sizeof(AseSeedsArg) == offsetof(AseSeedsArg, tabs) + sizeof(SeedTabs),
              "nesting SeedTabs moves no byte of the argument block");
struct AseSeedsKArg {
    FreqHot hot;
    FreqCold cold;
    AseSeedsArg set;
};
typedef const RT_CONST_AS AseSeedsArg *AsePtr;

template <int SF>
__device__ __forceinline__ void step_ase_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, AsePtr Q, const int n_seed, double *lds_iang,
                                                    double *lds_ev, const double *tab, double *xpose, const unsigned tile, const int lane)
{
    constexpr int NS      = RT_N_SEED_MAX;
    constexpr bool EMIS   = true; // (rt_tile_batch.inc: record 0 is the emission text)
    const int S           = SF ? SF : H.L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned ridx   = tile * WAVE + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = H.method == 1;
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool safe_check = (hflags & FQ_SAFE_CHECK) != 0, safe_skip = (hflags & FQ_SAFE_SKIP) != 0;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;

    // ---- per-ray preamble, once: exit ray, deposit cells (rt_tile_ray.inc, place_ray without its seed half) ----
#define TILE_NEED_RAY (!(hflags & FQ_OWN_CELLS) || probe_on)
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    int pix = -1, ang = -1;
    if (have && !err1) {
        const Placed P = place_ray(hflags & ~(unsigned) FQ_HAS_SEED, C, R, H.nx, backward, ridx, m, fl, ray);
        pix = P.pix;
        ang = P.ang;
    }
    if (have && probe_on) {
        C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
        C->probe.steps[ridx] = steps;
    }
    if (err1 && !safe_skip) { // error -1: the ray is reported (once), deposits into no record, and every record's code has the bit
        report_failure(1u << 1);
#pragma unroll
        for (int r = 0; r < 1 + NS; r++)
            if (r <= n_seed)
                atomicOr(&H.ctl->rec_code[r], 1u << 1);
    }
    const unsigned all_recs = (2u << n_seed) - 1u;
    // bit r: the lane's ray is live under record r (one word per lane, not a lane mask per record).  Not under the records
    // the checking pass found it failing in; record 0: rt_step_kernel's live mask; the seed records: F_SKIP does not count
    unsigned live = 0u;
    if (have && !err1) {
        live = all_recs & ~(safe_skip ? (unsigned) H.bad[ridx] : 0u);
        if (fl & F_SKIP)
            live &= ~1u;
    }
    if (__ballot(live != 0u) == 0ull)
        return;
    if (live == 0u) {
        pix = -1;
        ang = -1;
    }
    const bool any0 = __ballot((live & 1u) != 0u) != 0ull; // (else rt_step_kernel returns here: no recurrence, nothing into record 0)

    // ---- the march record of this lane's ray and the tile-wide choice of the update, once (rt_tile_rec.inc): over every
    // lane that holds a ray, as in rt_step_kernel ----
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
    const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;
    // (the gain-only half of rt_tile_batch.inc is dead text here, EMIS is true: what it names)
    constexpr double f0 = 0.0;
    const ConstF64 sfk  = dv2;

    // ---- per seed: the seed factor f0_s of the lane's ray, place_ray's arithmetic and order (Helper.h:523-533), as
    // step_seeds_tile computes it.  Run at the head of the seed half, and from the record and the launch ray read again
    // there: nothing of it is then live across the emission loop of SF = 6 (HALVES, below) ----
    double fs[NS];
    auto seed_factors = [&]() {
#pragma unroll
        for (int s = 0; s < NS; s++)
            fs[s] = 0.0;
        if (!(live >> 1) || (fl & F_ESCAPED)) // (live under no seed: whatever the lane integrates is dropped)
            return;
        const double *sf0 = Q->tabs.sf[0]; // (the tables of the seeds exist on a forward ray grid, for all seeds or none)
        if (backward || !sf0) {
            double qx, qy, qa, qb;
            if (backward) { // the exit ray, Helper.h:518-521: atanf(s.x / s.z) * 1e3f
                const RecMeta mm = *reinterpret_cast<const RecMeta *>(rec + rec_meta_off(rrec, S, H.rec_stride));
                qx = (double) mm.px;
                qy = (double) mm.py;
                qa = (double) (atanf_flt32_kernel(mm.sx / mm.sz) * 1e3f);
                qb = (double) (atanf_flt32_kernel(mm.sy / mm.sz) * 1e3f);
            } else { // the launch ray
                rt_ray lr = { 0, 0, 0, 0 };
                float ta, tb;
                load_ray(R, ridx, lr, ta, tb, false);
                qx = (double) lr.x;
                qy = (double) lr.y;
                qa = (double) lr.a;
                qb = (double) lr.b;
            }
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const DevSeed SD = load_cold(&Q->tabs.seed[s]);
                    fs[s]            = seed_factor(SD, qx, qy, qa, qb);
                }
            }
        } else {
            // the launch ray is a grid point: product of the seed's tabulated factors (RT_SEED_GRID_FACTOR)
            RT_SEED_GRID_POINT(R, ridx)
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const double *sf         = Q->tabs.sf[s];
                    const unsigned char *sin = Q->tabs.sin[s];
                    RT_SEED_GRID_FACTOR(fs[s], Q->tabs.seed[s].f0, sf, sin)
                }
            }
        }
    };

    // per record: RayTraceImageCPU.cpp:63-68 sequential in k, and min over k of Iv (Helper.h:582-594); index 0 is ASE
    double angsum[1 + NS], iv_min[1 + NS];
#pragma unroll
    for (int r = 0; r < 1 + NS; r++) {
        angsum[r] = 0.0;
        iv_min[r] = 0.0;
    }
    unsigned neg = 0u; // bit r: iv_min[r] < 0, taken at the end of the half that integrates record r

    // SF = 6: two loops over kb, the emission half, then the seed half (the head of this file says why); generic S: one
    constexpr int HALVES = SF ? 2 : 1;
#pragma unroll
    for (int half = 0; half < HALVES; half++) {
        const bool do_ase = any0 && half == 0, do_seeds = half == HALVES - 1;
        if (!do_ase && !do_seeds)
            continue;
        // (the gain sums of the seed half opaque at its head: (double) gs[s] is invariant in kb, and computed ahead of the
        // emission loop its six doubles were live across it -- 132 VGPRs where the two halves alone take 116 and 102)
        float gq[SF ? SF : 1];
        if (do_seeds) {
            seed_factors();
#pragma unroll
            for (int s = 0; s < (SF ? SF : 1); s++) {
                gq[s] = gs[s];
                asm volatile("" : "+v"(gq[s]));
            }
        }
        for (int kb = 0; kb < K; kb += VEC) {
            // the rows of this batch (generic S: row by row inside the emission loop, once for both halves)
            FVec w[SF ? SF : 1];
            if (SF)
                load_rows(w, kb);
            double gl[VEC]; // gain only, Helper.h:569-580: f64 products summed in sub-segment order
#pragma unroll
            for (int j = 0; j < VEC; j++)
                gl[j] = 0.0;
            double Iv[VEC];
            if (do_ase) {
                // ---- record 0: the emission recurrence (rt_tile_batch.inc, its EMIS text) ----
#define TILE_READ_SLOT rec_slot_lazy
#define TILE_REREAD have
#define TILE_BATCH_ROWS_LOADED
#define TILE_BATCH_SLOT(g, row)                                                                                                        \
        _Pragma("unroll") for (int j = 0; j < VEC; j++) gl[j] += (double) (g) * (double) (row).v[j];
#include "rt_tile_batch.inc"
#undef TILE_READ_SLOT
#undef TILE_REREAD
#undef TILE_BATCH_ROWS_LOADED
#undef TILE_BATCH_SLOT
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    iv_min[0] = fmin(iv_min[0], Iv[j]);
                    angsum[0] += dv2[kb + j] * Iv[j]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                }
                if (!safe_check) { // the checking pass of a failing run integrates without depositing
                    const bool dep_0 = pix >= 0 && (live & 1u);
#define EV_SUM_DEPOSITS dep_0
#define EV_SUM_INDEX kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
                }
            }
            if (!do_seeds)
                continue;
            // ---- the seed records: gl[] of the same rows, one exponential for all seeds (the text of rt_step_seeds.hip) ----
            if (SF) {
#pragma unroll
                for (int s = 0; s < SF; s++) {
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        gl[j] += (double) gq[s] * (double) w[s].v[j];
                }
            } else if (!do_ase) { // (generic S: the emission loop did not run, its slot hook has not summed)
                for (int s = 0; s < S; s++) {
                    const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
                    const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                    const FVec wr    = *reinterpret_cast<const FVec *>(row);
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        gl[j] += (double) sl.g * (double) wr.v[j];
                }
            }
            // Iv_s = f0_s f_s[4][k] exp(gl); for f0_s = 0 that is exactly 0 unless exp overflows (0 * inf): a wave none of whose
            // lanes needs the exponential under any seed skips it
            bool need = false;
#pragma unroll
            for (int s = 0; s < NS; s++)
                need = need || fs[s] != 0.0;
#pragma unroll
            for (int j = 0; j < VEC; j++)
                need = need || gl[j] > 700.0 || gl[j] != gl[j];
            const bool with_exp = __ballot(need) != 0ull;
            double eg[VEC];
#pragma unroll
            for (int j = 0; j < VEC; j++)
                eg[j] = 1.0;
            if (with_exp)
                exp_tab_vec(gl, tab, eg);
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const ConstF64 sk = (ConstF64) (unsigned long long) Q->tabs.fk[s];
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        Iv[j] = fs[s] * sk[kb + j];
                    if (with_exp) {
#pragma unroll
                        for (int j = 0; j < VEC; j++)
                            Iv[j] *= eg[j];
                    }
#pragma unroll
                    for (int j = 0; j < VEC; j++) {
                        iv_min[1 + s] = fmin(iv_min[1 + s], Iv[j]);
                        angsum[1 + s] += dv2[kb + j] * Iv[j]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                    }
                    if (!safe_check) {
                        // E_v of seed s: the wave sum over the lanes that deposit under this seed, its scale, its accumulator
                        const bool dep_s = pix >= 0 && ((live >> (1 + s)) & 1u);
                        const double scale_s = Q->scale[1 + s];
#define EV_SUM_DEPOSITS dep_s
#define EV_SUM_INDEX (1 + s) * Kp + kb
#define EV_SUM_SCALE scale_s
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
#undef EV_SUM_SCALE
                    }
                }
            }
        }
        if (do_ase)
            neg |= iv_min[0] < 0.0 ? 1u : 0u;
        if (do_seeds) {
#pragma unroll
            for (int s = 0; s < NS; s++)
                neg |= iv_min[1 + s] < 0.0 ? 2u << s : 0u;
        }
    }
    // per record: a negative intensity is error -2, a NaN in the I_ang sum error -3, after the sign test (Helper.h:582-594);
    // only of a ray that is live under the record (what any other lane integrated is dropped)
    unsigned failing = 0u, code = 0u;
#pragma unroll
    for (int r = 0; r < 1 + NS; r++) {
        if (r <= n_seed) {
            const bool bad_neg = ((neg >> r) & 1u) != 0u, bad_nan = angsum[r] != angsum[r];
            if (((live >> r) & 1u) && (bad_neg || bad_nan)) {
                failing |= 1u << r;
                if (!safe_skip) {
                    const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                    code |= c;
                    atomicOr(&H.ctl->rec_code[r], c);
                }
            }
        }
    }
    if (code) { // (not the skipping pass) one report per ray, whatever the number of records it fails under
        report_failure(code);
        if (safe_check)
            H.bad[ridx] = (unsigned char) failing; // the lane that holds the ray writes all its bits
    }
    if (safe_check)
        return;
    // runs of lanes with equal pixel, found once for all records (rt_wave_runs.inc); the last lane of a run owns the total
#define RUNS_PIX pix
#define RUNS_DEPOSITS (pix >= 0)
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
#pragma unroll
    for (int r = 0; r < 1 + NS; r++) {
        if (r <= n_seed) {
            // a ray that fails under record r adds nothing to record r (RayTraceImageCPU.cpp:29-36: `continue` before the deposit)
            const bool ok = ((live & ~failing) >> r) & 1u;
            if (ang >= 0 && ok) {
                if (lds_iang)
                    unsafeAtomicAdd(&lds_iang[r * seeds_ang_stride(H.n_ang) + ang], angsum[r]);
                else
                    unsafeAtomicAdd(&Q->out[r].iang[ang], angsum[r]);
            }
            double a = (pix >= 0 && ok) ? angsum[r] * Q->scale[r] : 0.0;
#include "rt_wave_runscan.inc"
            if (tail && a != 0.0)
                unsafeAtomicAdd(&Q->out[r].nf[pix], a);
        }
    }
}

// The shell of rt_step_kernel (rt_step_wg.inc, rt_step_handout.inc) with 1 + n_seed records: per record an I_ang histogram,
// seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.  The register budget of rt_step_kernel<SF, true>.
template <int SF>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES) rt_step_ase_seeds_kernel(const AseSeedsKArg A)
{
    const FreqHot &H = A.hot;
#define STEP_WG_NREC 1 + A.set.n_seed
#define STEP_WG_ANG_STRIDE seeds_ang_stride(n_ang)
#define STEP_WG_ANG_ZERO n_rec * ang_stride
#define STEP_WG_RECORD(r)
#define STEP_WG_EV(r, c) A.set.out[r].E_v[c]
#define STEP_WG_IANG(r, c) A.set.out[r].iang[c]
#define STEP_WG_PROLOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_PROLOGUE
    const int lane = lane_id();
    // the cold half and the seeds of the argument block, the flag word and the lane number opaque per tile
#define HANDOUT_TILES_PER_FETCH FREQ_TILES_PER_FETCH_EMIS
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(AseSeedsKArg, cold));        \
    AsePtr Q  = (AsePtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(AseSeedsKArg, set));           \
    asm volatile("" : "+s"(C), "+s"(Q));                                                                                               \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    asm volatile("" : "+s"(hflags), "+v"(lane_t));                                                                                     \
    step_ase_seeds_tile<SF>(H, hflags, C, Q, n_rec - 1, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
#include "rt_step_handout.inc"
#undef HANDOUT_TILES_PER_FETCH
#undef HANDOUT_TILE
#define STEP_WG_EPILOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_EPILOGUE
#undef STEP_WG_NREC
#undef STEP_WG_ANG_STRIDE
#undef STEP_WG_ANG_ZERO
#undef STEP_WG_RECORD
#undef STEP_WG_EV
#undef STEP_WG_IANG
}

} // namespace rt
