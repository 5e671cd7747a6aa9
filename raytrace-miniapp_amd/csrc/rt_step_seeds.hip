#pragma once
// rt_step_seeds.hip -- step mode with a seed set (rt_hip_plan_set_seeds): the records of up to RT_N_SEED_MAX seed beams
// from ONE march.
//
// The application's per-step record (intensity_step_struct, src/RayTraceStructures.h:361-369) holds one seeded triple
// E_v_seed[s], image_seed[s], E_ang_seed[s] per seed beam, s < N_seed <= N_SEED_MAX = 2.  The march record (gvl / evl /
// ivl, exit point, direction, flags) holds nothing of the seed (Helper.h:428-521): the seed enters in the frequency pass
// only, as Iv[k] = f0_s f_s[4][k] exp(gl[k]) (Helper.h:523-533, 569-580), and exp(gl[k]) is the same for every seed.
// rt_step_seeds_kernel stands where rt_step_kernel stands, gain-only, and has its shape: one 16-wave work-group per CU,
// tiles from the eight sharded counters, lanes = rays; the per-ray preamble (rt_tile_ray.inc) and the record decode
// (rt_tile_rec.inc) are the text rt_step.hip includes.  Per tile, once: preamble, decode, pixel and angle cell (place_ray
// without its seed half).  Per seed: f0_s in place_ray's own arithmetic and order -- on a forward ray grid the product of
// the seed's tabulated factors with the clamp, otherwise seed_factor on the seed's DevSeed.  Per frequency batch: gl[] and
// exp_tab_vec once (needed if any seed's f0 != 0, or gl > 700, or gl is a NaN), then per seed in turn
// Iv_s[j] = (f0_s sfk_s[kb + j]) eg[j] -- the double rt_step_kernel computes for that seed, in its association -- the lane's
// sums and the E_v wave sum (rt_step_evsum.inc) into the seed's accumulator in LDS; only f0_s, angsum_s and iv_min_s are
// live per seed.  Per tile end and seed: the I_ang add and the segmented nf scan (rt_wave_runscan.inc over the runs of equal
// pixel, which rt_wave_runs.inc finds once).  The kernel's shell -- LDS, prologue, epilogue, tile hand-out -- is the text
// rt_step_kernel includes (rt_step_wg.inc, rt_step_handout.inc), the grid-point seed factor the macro place_ray expands
// (RT_SEED_GRID_FACTOR, rt_freq.hip).
//
// Failures follow the reference run once per seed: error -1 does not depend on the seed (the ray deposits into no record,
// every seed's code carries the bit); error -2 / -3 under seed s removes the ray from record s only
// (RayTraceImageCPU.cpp:29-36 per create_image call).  The checking repeat (plan_repeat_checked) keeps its two passes; the
// mark of a ray in bad[] is one bit per seed, written by the one lane that holds the ray.  A ray that fails under any seed
// is reported once, with the OR of its codes, into the control block; DevCtl::seed_code[s] holds the code of seed s.
#include "rt_step.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

// the record of one seed: E_v [K], nf [nx * ny], I_ang [na * nb] inside the plan's one allocation
struct SeedRec {
    double *E_v, *nf, *iang;
};
// the tables of the seeds of a pass: the last member of SeedSetArg, ScanSeedsArg (rt_step_scan_seeds.hip) and AseSeedsArg
// (rt_step_ase_seeds.hip), filled by one function of rt_launch.hip
struct SeedTabs {
    const double *fk[RT_N_SEED_MAX];         // [Kp] f[4] of the seed, zero padded
    const double *sf[RT_N_SEED_MAX];         // forward ray grid: the seed's factor tables (rt_seed_tab_kernel), else NULL
    const unsigned char *sin[RT_N_SEED_MAX]; // ... and its support flags
    DevSeed seed[RT_N_SEED_MAX];
};
// what rt_step_seeds_kernel reads beside the frequency kernel's block: read through the constant address space where it
// is needed (as the cold half is), so that nothing of it is live across the frequency loop
struct SeedSetArg {
    int n_seed;
    int pad;
    SeedRec out[RT_N_SEED_MAX];
    SeedTabs tabs;
};
static_assert(offsetof(SeedSetArg, tabs) == 8 + sizeof(SeedRec) * RT_N_SEED_MAX && offsetof(SeedTabs, fk) == 0 &&
                  offsetof(SeedTabs, seed) == 3 * sizeof(void *) * RT_N_SEED_MAX && sizeof(SeedSetArg) == offsetof(SeedSetArg, tabs) + sizeof(SeedTabs),
              "nesting SeedTabs moves no byte of the argument block");
struct SeedsKArg {
    FreqHot hot;
    FreqCold cold;
    SeedSetArg set;
};
typedef const RT_CONST_AS SeedSetArg *SetPtr;

template <int SF>
__device__ __forceinline__ void step_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SetPtr Q, const int n_seed, double *lds_iang,
                                                double *lds_ev, const double *tab, double *xpose, const unsigned tile, const int lane)
{
    constexpr int NS      = RT_N_SEED_MAX;
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
    double f0[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        f0[s] = 0.0;
    int pix = -1, ang = -1;
    if (have && !err1) {
        const Placed P = place_ray(hflags & ~(unsigned) FQ_HAS_SEED, C, R, H.nx, backward, ridx, m, fl, ray);
        pix = P.pix;
        ang = P.ang;
        // ---- per seed: the seed factor, place_ray's arithmetic and order (Helper.h:523-533) ----
        if (!(fl & F_ESCAPED)) {
            if (backward || !R.sf) {
                float ra = 0.0f, rb = 0.0f;
                if (backward) { // Helper.h:518-521: atanf(s.x / s.z) * 1e3f
                    ra = atanf_flt32_kernel(m.sx / m.sz) * 1e3f;
                    rb = atanf_flt32_kernel(m.sy / m.sz) * 1e3f;
                }
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
                        const DevSeed SD = load_cold(&Q->tabs.seed[s]);
                        f0[s] = backward ? seed_factor(SD, (double) m.px, (double) m.py, (double) ra, (double) rb)
                                         : seed_factor(SD, (double) ray.x, (double) ray.y, (double) ray.a, (double) ray.b);
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
                        RT_SEED_GRID_FACTOR(f0[s], Q->tabs.seed[s].f0, sf, sin)
                    }
                }
            }
        }
    }
    if (have && probe_on) {
        C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
        C->probe.steps[ridx] = steps;
    }
    if (err1 && !safe_skip) { // error -1: the ray is reported (once), deposits into no record, and every seed's code has the bit
        report_failure(1u << 1);
#pragma unroll
        for (int s = 0; s < NS; s++)
            if (s < n_seed)
                atomicOr(&H.ctl->seed_code[s], 1u << 1);
    }
    const unsigned all_seeds = (1u << n_seed) - 1u;
    // the seeds under which the checking pass found this ray failing: it stays out of their records
    const unsigned marked = (safe_skip && have) ? ((unsigned) H.bad[ridx] & all_seeds) : 0u;
    const bool live       = have && !err1 && !(fl & F_SKIP) && marked != all_seeds;
    if (__ballot(live) == 0ull)
        return;
    if (!live) {
        pix = -1;
        ang = -1;
    }

    // ---- the march record of this lane's ray and the tile-wide choice of the update, once (rt_tile_rec.inc) ----
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
    (void) rs;
    (void) all_small;
    (void) gv_nan;
    const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;

    double angsum[NS], iv_min[NS]; // per seed: RayTraceImageCPU.cpp:63-68 sequential in k, and min over k of Iv (Helper.h:582-594)
#pragma unroll
    for (int s = 0; s < NS; s++) {
        angsum[s] = 0.0;
        iv_min[s] = 0.0;
    }
    const bool dep = pix >= 0; // this lane's ray deposits into the images of the seeds it is not marked under

    for (int kb = 0; kb < K; kb += VEC) {
        // gain only, Helper.h:569-580: f64 products summed in sub-segment order (the text of rt_tile_batch.inc); once
        double gl[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            gl[j] = 0.0;
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
                const ConstF64 sfk = (ConstF64) (unsigned long long) Q->tabs.fk[s];
                double Iv[VEC];
#pragma unroll
                for (int j = 0; j < VEC; j++)
                    Iv[j] = f0[s] * sfk[kb + j];
                if (with_exp) {
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        Iv[j] *= eg[j];
                }
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    iv_min[s] = fmin(iv_min[s], Iv[j]);
                    angsum[s] += dv2[kb + j] * Iv[j]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                }
                if (!safe_check) { // the checking pass of a failing run integrates without depositing
                    // E_v of seed s: the wave sum over the lanes that deposit under this seed, into the seed's accumulator
                    const bool dep_s = dep && !((marked >> s) & 1u);
#define EV_SUM_DEPOSITS dep_s
#define EV_SUM_INDEX s * Kp + kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
                }
            }
        }
    }
    // per seed: a negative intensity is error -2, a NaN in the I_ang sum error -3, after the sign test (Helper.h:582-594)
    unsigned failing = 0u, code = 0u;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            const bool bad_neg = iv_min[s] < 0.0, bad_nan = angsum[s] != angsum[s];
            if (bad_neg || bad_nan) {
                failing |= 1u << s;
                if (live && !safe_skip) {
                    const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                    code |= c;
                    atomicOr(&H.ctl->seed_code[s], c);
                }
            }
        }
    }
    if (code) { // (live, not the skipping pass) one report per ray, whatever the number of seeds it fails under
        report_failure(code);
        if (safe_check)
            H.bad[ridx] = (unsigned char) failing; // the lane that holds the ray writes all its bits
    }
    if (safe_check)
        return;
    // runs of lanes with equal pixel, found once for all seeds (rt_wave_runs.inc); the last lane of a run owns the total
#define RUNS_PIX pix
#define RUNS_DEPOSITS dep
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            // a ray that fails under seed s adds nothing to record s (RayTraceImageCPU.cpp:29-36: `continue` before the deposit)
            const bool ok = !((failing >> s) & 1u) && !((marked >> s) & 1u);
            if (ang >= 0 && ok) {
                if (lds_iang)
                    unsafeAtomicAdd(&lds_iang[s * seeds_ang_stride(H.n_ang) + ang], angsum[s]);
                else
                    unsafeAtomicAdd(&Q->out[s].iang[ang], angsum[s]);
            }
            double a = (dep && ok) ? angsum[s] * H.scale : 0.0;
#include "rt_wave_runscan.inc"
            if (tail && a != 0.0)
                unsafeAtomicAdd(&Q->out[s].nf[pix], a);
        }
    }
}

// The shell of rt_step_kernel (rt_step_wg.inc, rt_step_handout.inc) with one record per seed: per seed an I_ang histogram,
// seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.
template <int SF>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_step_seeds_kernel(const SeedsKArg A)
{
    const FreqHot &H = A.hot;
#define STEP_WG_NREC A.set.n_seed
#define STEP_WG_ANG_STRIDE seeds_ang_stride(n_ang)
#define STEP_WG_ANG_ZERO n_rec * ang_stride
#define STEP_WG_RECORD(r)
#define STEP_WG_EV(r, c) A.set.out[r].E_v[c]
#define STEP_WG_IANG(r, c) A.set.out[r].iang[c]
#define STEP_WG_PROLOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_PROLOGUE
    const int lane = lane_id();
    // the cold half and the seed set of the argument block, the flag word and the lane number opaque per tile
#define HANDOUT_TILES_PER_FETCH FREQ_TILES_PER_FETCH_GAIN
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SeedsKArg, cold));           \
    SetPtr Q  = (SetPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SeedsKArg, set));              \
    asm volatile("" : "+s"(C), "+s"(Q));                                                                                               \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    asm volatile("" : "+s"(hflags), "+v"(lane_t));                                                                                     \
    step_seeds_tile<SF>(H, hflags, C, Q, n_rec, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
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
