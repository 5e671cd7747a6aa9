#pragma once
// rt_spec_ase_seeds.hip -- spectra mode of an EMISSION plan that carries ASE seeds (rt_hip_plan_set_spectra_ase_seeds):
// RayTrace::calc_ray of the ASE problem AND of the same problem under up to RT_N_SEED_MAX seed beams, for every ray of a run,
// from ONE march and ONE pass over the march record.
//
// The premise is that of rt_step_ase_seeds.hip: the trajectory, gvl, the exit state, the escape flag and the step count do
// not depend on use_emis; only evl does.  The march record of an emission plan therefore holds everything the gain-only pass
// of a seeded run of the same problem reads, and rt_spec_ase_seeds_kernel<SF> leaves 1 + n_seed row blocks from it:
//   block 0       the row rt_spec_kernel<SF, true> leaves on this plan: the emission recurrence, the text of rt_tile_batch.inc
//                 over the decode of rt_tile_rec.inc with the mask spec_tile passes (have && !err1 && !F_SKIP), so the
//                 tile-wide choice is taken over the same lanes; exact emission and gv_nan included
//   block 1 + s   the row rt_spec_kernel<SF, false> leaves of the same problem created with seed s (E0 present and unused):
//                 gain-only, Iv[k] = (f0_s f_s[4][k]) exp(gl[k]), in the association and with the exponential-skip rule of
//                 rt_spec_seeds.hip (`need` over all seeds)
// It stands where rt_spec_kernel stands and has the shell of rt_spec_seeds_kernel: one 16-wave work-group per CU, tiles from
// the eight sharded counters, lanes = rays, the two exponent tables and ONE [64][XS_ROW] staging per wave in LDS.
//
// Per tile, once: the tile head of spectra mode (rt_spec_tile.inc, SPEC_TILE_HEAD: the preamble, the -1 test, the exit ray, the
// probe) and the record decode.  Then two halves over the frequencies, the HALVES of rt_step_ase_seeds.hip, both the text of
// rt_spec_tile.inc:
//   emission half  SPEC_TILE_EMISSION, the loop spec_tile<SF, true> includes: 16 values of 64 rows staged, 128-byte row
//                  segments into block 0
//   seed half      SPEC_TILE_SEEDS, the loop spec_seeds_tile<SF> includes: the seed factors first (SPEC_TILE_FACTORS: forward at
//                  the launch ray -- on a ray grid the product of the seed's tabulated factors --, backward at the exit state;
//                  taken here so that nothing of them is live across the emission loop), then the exponentials and f0_s staged,
//                  the storing lanes forming the products on the way out into blocks 1 + s
// The seed half reads the lineshape rows again, from the caches.  This file's own are the statements between the halves: where
// the seeds are taken (the record and the launch ray read again), the live mask and the staging of the factors, the pins
// of the gain sums.
//
// F_SKIP: the emission march marks a ray whose every gvl / evl sum is zero (never when a lineshape table holds a non-finite
// value, DevParams::no_skip).  It gets a row of zeros in block 0, as in rt_spec_kernel; under a seed it is live and carries
// f0_s f_s[4][k] exp(0).  Its zeroed slots and its real slots both give gl = +0 (its gs are all +0), so the one decode serves
// both halves.  A tile none of whose rays is live for block 0 skips the recurrence, writes block 0's zeros and runs the seed half.
//
// Outputs, block-major in the one allocation of the mode: Iv [1 + n_seed][n_rays][K] (row stride K), err [1 + n_seed][n_rays],
// ray2 [n_rays].  Error -1 and the exit ray do not depend on the block; -2 / -3 are per block, -2 wins.  Every element is written.
// Failures: a ray is reported once with the OR of its codes over the blocks; DevCtl::rec_code[r] carries the code of block r.
// Nothing is deposited: no checking repeat.
#include "rt_spec_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_spec.hip: the same contractions, the same doubles)

// the argument block is that of rt_spec_seeds_kernel: out holds 1 + n_seed blocks here
template <int SF>
__device__ __forceinline__ void spec_ase_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SpecSeedsPtr Q, const int n_seed, const double *tab,
                                                    double *stage, const unsigned tile, const int lane)
{
    constexpr int NS    = RT_N_SEED_MAX;
    constexpr bool EMIS = true; // (rt_tile_batch.inc: block 0 is the emission text)

    // ---- the tile head, once (rt_spec_tile.inc) ----
#define SPEC_TILE_HEAD
#define SPEC_TILE_NEED_RAY false // (the seed half reads the launch ray where it needs it)
#define SPEC_TILE_RAY2 Q->out.ray2
#define SPEC_TILE_ERR1_CODES /* every block's code has the bit */                                                              \
    _Pragma("unroll") for (int r = 0; r < 1 + NS; r++) if (r <= n_seed) atomicOr(&H.ctl->rec_code[r], 1u << 1);
#include "rt_spec_tile.inc"
#undef SPEC_TILE_ERR1_CODES
#undef SPEC_TILE_RAY2
#undef SPEC_TILE_NEED_RAY
#undef SPEC_TILE_HEAD
    // block 0: spec_tile's live mask -- a ray with error -1, and one whose every update is the identity (F_SKIP), gets a row
    // of zeros; the seed blocks: F_SKIP does not count
    const bool live     = have && !err1 && !(fl & F_SKIP);
    const bool any_live = __ballot(live) != 0ull;
    const bool lives    = have && !err1;

    // ---- the march record of this lane's ray, the slots of a lane without a ray live for block 0 zeroed (as spec_tile) ----
#define TILE_MASK live
#include "rt_tile_rec.inc"
#undef TILE_MASK
    // (the gain-only half of rt_tile_batch.inc is dead text here, EMIS is true: what it names)
    constexpr double f0 = 0.0;
    const ConstF64 sfk  = (ConstF64) (unsigned long long) H.seed_fk;

    // a full tile and an even K: every 16-frequency group that lies inside K leaves as 16-byte stores
    const bool wide_ok    = row0 + WAVE <= n_rays && (K & 1) == 0;
    const size_t blk_rows = (size_t) n_rays; // rows of one block
    unsigned code = 0u;

    // ================= the emission half: block 0, the loop of spec_tile<SF, true> =================
    {
        double *Iv0 = Q->out.Iv;
#define SPEC_TILE_EMISSION
#define SPEC_TILE_IV Iv0
#include "rt_spec_tile.inc"
#undef SPEC_TILE_IV
#undef SPEC_TILE_EMISSION
        const bool bad_neg = live && iv_min < 0.0, bad_nan = live && has_nan;
        if (have)
            Q->out.err[ridx] = err1 ? -1 : (bad_neg ? -2 : (bad_nan ? -3 : 0));
        if (bad_neg || bad_nan) {
            code = bad_neg ? (1u << 2) : (1u << 3);
            atomicOr(&H.ctl->rec_code[0], code);
        }
    }

    // ================= the seed half: blocks 1 + s, the loop of spec_seeds_tile<SF> =================
    // ---- per seed: the seed factor, as spec_seeds_tile takes it: from the record and the launch ray read again here ----
    double fs[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        fs[s] = 0.0;
    if (lives && !(fl & F_ESCAPED)) {
        const double *sf0 = Q->tabs.sf[0]; // (the tables of the seeds exist on a forward ray grid, for all seeds or none)
#define SPEC_TILE_FACTORS
#define SPEC_TILE_FS fs
#define SPEC_TILE_AT_POINT (backward || !sf0)
#define SPEC_TILE_POINT                                                                                                        \
    double px, py, pa, pb;                                                                                                     \
    if (backward) { /* the exit state, Helper.h:518-521 */                                                                     \
        const RecMeta mm = *reinterpret_cast<const RecMeta *>(rec + rec_meta_off(rrec, S, H.rec_stride));                      \
        px = (double) mm.px;                                                                                                   \
        py = (double) mm.py;                                                                                                   \
        pa = (double) (atanf_flt32_kernel(mm.sx / mm.sz) * 1e3f);                                                              \
        pb = (double) (atanf_flt32_kernel(mm.sy / mm.sz) * 1e3f);                                                              \
    } else { /* the launch ray */                                                                                              \
        rt_ray lr = { 0, 0, 0, 0 };                                                                                            \
        float ta, tb;                                                                                                          \
        load_ray(R, ridx, lr, ta, tb, false);                                                                                  \
        px = (double) lr.x;                                                                                                    \
        py = (double) lr.y;                                                                                                    \
        pa = (double) lr.a;                                                                                                    \
        pb = (double) lr.b;                                                                                                    \
    }
#include "rt_spec_tile.inc"
#undef SPEC_TILE_POINT
#undef SPEC_TILE_AT_POINT
#undef SPEC_TILE_FS
#undef SPEC_TILE_FACTORS
    }
    const bool any_lives = __ballot(lives) != 0ull;
    // what the storing lanes need of a row beside its exponentials: whether it is live, and its seed factors -- once per tile
    // (the last flush of the emission half ended behind a wave barrier; the first flush of this half begins behind one)
    const unsigned long long live_mask = __ballot(lives);
#pragma unroll
    for (int s = 0; s < NS; s++)
        stage[lane * XS_ROW + SPEC_SEEDS_F0 + s] = fs[s];
    // (the gain sums opaque at the head of this half: (double) gs[s] is invariant in kb -- rt_step_ase_seeds.hip)
    float gq[SF ? SF : 1];
#pragma unroll
    for (int s = 0; s < (SF ? SF : 1); s++) {
        gq[s] = gs[s];
        asm volatile("" : "+v"(gq[s]));
    }

    // ---- the frequencies, gain only, and the codes per seed block; a failing ray is reported once, with the codes of all blocks ----
#define SPEC_TILE_SEEDS
#define SPEC_TILE_FS fs
#define SPEC_TILE_LIVE lives
#define SPEC_TILE_ANY_LIVE any_lives
#define SPEC_TILE_GS gq
#define SPEC_TILE_BLOCK(s) 1 + s
#define SPEC_TILE_CODE(s) H.ctl->rec_code[1 + s]
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

// The shell of rt_spec_seeds_kernel (and its argument block): one work-group of FREQ_WG_WAVES waves per CU, tiles from the eight
// sharded counters, one tile per fetch; LDS, all dynamic: the two exponent tables, then [64][XS_ROW] staging doubles per wave.
// The register budget of rt_spec_kernel<SF, true>.
template <int SF>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES) rt_spec_ase_seeds_kernel(const SpecSeedsKArg A)
{
    const int n_seed = A.set.n_seed;
#define SPEC_WG_KERNEL
#define SPEC_WG_KARG SpecSeedsKArg
#define SPEC_WG_BLOCK set
#define SPEC_WG_BLOCK_PTR SpecSeedsPtr
#define SPEC_WG_CALL spec_ase_seeds_tile<SF>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_CALL
#undef SPEC_WG_BLOCK_PTR
#undef SPEC_WG_BLOCK
#undef SPEC_WG_KARG
#undef SPEC_WG_KERNEL
}

} // namespace rt
