#pragma once
// rt_spec_seeds.hip -- spectra mode with the seeds of rt_hip_plan_set_spectra_seeds: RayTrace::calc_ray for every ray of a
// run under up to RT_N_SEED_MAX seed beams, from ONE march and ONE walk over the march record.
//
// The premise is that of rt_step_seeds.hip: neither the march record nor the exit ray holds anything of the seed, which
// enters as Iv_s[k] = (f0_s f_s[4][k]) exp(gl[k]) only (Helper.h:523-533, 569-580).  rt_spec_seeds_kernel<SF> stands where
// rt_spec_kernel<SF, false> stands, gain-only, and has its shell, its LDS and its launch bounds.  Per tile, once: the tile
// head of spectra mode (rt_spec_tile.inc, SPEC_TILE_HEAD: the preamble, the -1 test, the exit ray) and the record decode
// (rt_tile_rec.inc, the slots of a lane without a live ray zeroed as spec_tile zeroes them).  Per seed: f0_s, in the order of
// step_seeds_tile -- forward at the launch ray (on a ray grid the product of the seed's tabulated factors), backward at the
// exit state (SPEC_TILE_FACTORS).  Per frequency batch (SPEC_TILE_SEEDS): gl[] and exp_tab_vec once -- needed if any seed's
// f0 != 0, or gl > 700, or gl is a NaN, the rule of rt_tile_batch.inc with `need` taken over all seeds as rt_step_seeds.hip
// argues -- then per seed Iv_s[j] = (f0_s sfk_s[kb + j]) eg[j], the double rt_spec_kernel computes on a plan created with
// seed s, in its association; the lane's -2 / -3 scan per seed (Helper.h:582-593: a negative value wins over a NaN).
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
    constexpr int NS = RT_N_SEED_MAX;
    double f0[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        f0[s] = 0.0;

    // ---- the tile head, once (rt_spec_tile.inc); per seed the seed factor, forward at the launch ray, backward at the exit state ----
#define SPEC_TILE_HEAD
#define SPEC_TILE_NEED_RAY (!backward) // the forward seed factors are taken at the launch ray
#define SPEC_TILE_RAY2 Q->out.ray2
#define SPEC_TILE_HEAD_FACTORS
#define SPEC_TILE_FS f0
#define SPEC_TILE_AT_POINT (backward || !R.sf)
#define SPEC_TILE_POINT                                                                                                        \
    const double px = backward ? (double) m.px : (double) ray.x, py = backward ? (double) m.py : (double) ray.y;               \
    const double pa = backward ? (double) r2.a : (double) ray.a, pb = backward ? (double) r2.b : (double) ray.b;
#define SPEC_TILE_ERR1_CODES /* every seed's code has the bit */                                                               \
    _Pragma("unroll") for (int s = 0; s < NS; s++) if (s < n_seed) atomicOr(&H.ctl->seed_code[s], 1u << 1);
#include "rt_spec_tile.inc"
#undef SPEC_TILE_ERR1_CODES
#undef SPEC_TILE_POINT
#undef SPEC_TILE_AT_POINT
#undef SPEC_TILE_FS
#undef SPEC_TILE_HEAD_FACTORS
#undef SPEC_TILE_RAY2
#undef SPEC_TILE_NEED_RAY
#undef SPEC_TILE_HEAD
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
    // a full tile and an even K: every group that lies inside K leaves as 16-byte stores
    const bool wide_ok    = row0 + WAVE <= n_rays && (K & 1) == 0;
    const size_t blk_rows = (size_t) n_rays; // rows of one seed's block
    unsigned code         = 0u;

    // ---- the frequencies, gain only, and the codes per seed (rt_spec_tile.inc); a failing ray is reported once ----
#define SPEC_TILE_SEEDS
#define SPEC_TILE_FS f0
#define SPEC_TILE_LIVE live
#define SPEC_TILE_ANY_LIVE any_live
#define SPEC_TILE_GS gs
#define SPEC_TILE_BLOCK(s) s
#define SPEC_TILE_CODE(s) H.ctl->seed_code[s]
#include "rt_spec_tile.inc"
#undef SPEC_TILE_CODE
#undef SPEC_TILE_BLOCK
#undef SPEC_TILE_GS
#undef SPEC_TILE_ANY_LIVE
#undef SPEC_TILE_LIVE
#undef SPEC_TILE_FS
#undef SPEC_TILE_SEEDS
    if (code)
        report_failure(code);
}

// The shell of rt_spec_kernel: one work-group of FREQ_WG_WAVES waves per CU, tiles from the eight sharded counters, one
// tile per fetch; LDS, all dynamic: the two exponent tables, then [64][XS_ROW] staging doubles per wave.
template <int SF>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_spec_seeds_kernel(const SpecSeedsKArg A)
{
    const int n_seed = A.set.n_seed;
#define SPEC_WG_KERNEL
#define SPEC_WG_KARG SpecSeedsKArg
#define SPEC_WG_BLOCK set
#define SPEC_WG_BLOCK_PTR SpecSeedsPtr
#define SPEC_WG_CALL spec_seeds_tile<SF>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_CALL
#undef SPEC_WG_BLOCK_PTR
#undef SPEC_WG_BLOCK
#undef SPEC_WG_KARG
#undef SPEC_WG_KERNEL
}

} // namespace rt
