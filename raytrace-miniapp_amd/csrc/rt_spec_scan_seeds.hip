#pragma once
// rt_spec_scan_seeds.hip -- length spectra with the seeds of rt_hip_plan_set_spectra_seeds: RayTrace::calc_ray for every ray
// at every plasma length n = 2 .. N under up to RT_N_SEED_MAX seed beams, from ONE scan march and ONE walk over the record.
//
// The premises are those of rt_spec_scan.hip and rt_step_scan_seeds.hip / rt_step_rscan_seeds.hip: the scan march leaves the
// state with which every ray crossed every length boundary, the table of rt_spec_scan.hip says which state serves row block
// n, and neither the march record nor those states hold anything of the seed, which enters as
// Iv_{s,n}[k] = (f0_{s,n} f_s[4][k]) exp(gl_n[k]) only.  rt_spec_scan_seeds_kernel<BACKWARD> stands where
// rt_spec_scan_kernel<false, BACKWARD> stands, gain-only, with its shell, LDS and launch bounds, and with its tile head, its
// serving state and its codes (rt_spec_scan_tile.inc); the seed factors are the text of spectra mode (rt_spec_tile.inc,
// SPEC_TILE_FACTORS), the walk and its stores that of rt_spec_scan_seeds_walk.inc.
//   forward   f0_s once per ray at the launch ray (on a ray grid the product of the seed's tabulated factors), 0 for the
//             blocks the ray has escaped by; one running gl per frequency batch, one exp_tab_vec per length for all seeds.
//   backward  the suffix walk of rt_spec_scan.hip with its shared product sums, SSS_LCH = 2 suffixes per walk (the single-seed
//             kernel walks four and sits at 127 VGPRs; two seeds double the factors and the values of a row, so the walk is
//             halved: the segments behind a chunk's last start are integrated once per chunk of two instead of once per chunk
//             of four -- for L = 5, 9 segment walks instead of 6, against 12 of two single-seed plans); f0[s][i] per (seed,
//             block of the chunk) at the state that serves the block (rscan_seed_factor on the seed where it lies in the
//             argument block: no copy of a DevSeed, no stack frame).
// The exponential of a row is skipped by a wave none of whose lanes needs it under any seed (rt_tile_batch.inc's rule with
// `need` over all seeds, as rt_step_seeds.hip argues); every Iv_{s,n}[k] is the double rt_spec_scan_kernel computes on a
// plan created with seed s, in its association.
//
// Outputs, seed-major then length-major: Iv [n_seed][L][n_rays][K] (row stride K), err [n_seed][L][n_rays], ray2 [L][n_rays]
// (error -1 and the exit ray do not depend on the seed).  Blocks 0 .. L - 1 are seed 0: the plain accessors of length spectra
// serve it.  Every element is written.
//
// The stores.  The staging row of a lane is cut into VEC frequencies of SSS_LCH = 2 lengths of RT_N_SEED_MAX = 2 seeds
// (column (li * 2 + s) * VEC + v): every piece stays the 32 bytes of rt_spec_scan.hip, 16 bytes per lane and 32 rows per
// instruction.  No slot is integrated twice for the stores' sake (the backward walk's halving is for the registers).
//
// Failures: a ray is reported once with the OR of its codes over all (seed, n); DevCtl::seed_code[s] carries the OR over n
// of seed s.  Nothing is deposited: no checking repeat.
#include "rt_spec_scan.hip"
#include "rt_step_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_spec.hip: the same contractions, the same doubles)

constexpr int SSS_LCH = 2; // lengths per staging and suffixes per backward walk
static_assert(SSS_LCH * RT_N_SEED_MAX * VEC <= XS_ROW - 2 && VEC == 4, "a staging row holds VEC frequencies of SSS_LCH lengths of every seed");

// what rt_spec_scan_seeds_kernel reads beside the frequency kernel's block (through the constant address space)
struct SpecScanSeedsArg {
    int n_seed;
    int pad;
    SpecOut out;              // Iv [n_seed][L][n_rays][K], ray2 [L][n_rays], err [n_seed][L][n_rays]
    const unsigned char *bnd; // boundary states of the march (scan_bnd_off)
    SeedTabs tabs;
};
struct SpecScanSeedsKArg {
    FreqHot hot;
    FreqCold cold;
    SpecScanSeedsArg set;
};
typedef const RT_CONST_AS SpecScanSeedsArg *SpecScanSeedsPtr;

template <bool BACKWARD>
__device__ __forceinline__ void spec_scan_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SpecScanSeedsPtr Q, const int n_seed,
                                                     const double *tab, double *stage, const unsigned tile, const int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH     = SSS_LCH;
    constexpr int NS      = RT_N_SEED_MAX;

    // ---- the tile head of length spectra, once: the final state of the ray, the segment it escaped in (rt_spec_scan_tile.inc) ----
#define SPEC_SCAN_HEAD
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_HEAD

#define SSS_WALK_F0
#define SSS_GRID_TABS R.sf
#include "rt_spec_scan_seeds_walk.inc"
#undef SSS_GRID_TABS
#undef SSS_WALK_F0

    // ---- the march record of this lane's ray (rt_tile_rec.inc; SF = 0: nothing to decode up front) ----
#define SPEC_SCAN_REC
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_REC

    // one bit per row block (bit m - 1 = block n - 2): error -1, live, not escaped (carries the seed factors); per seed: a
    // negative value seen, a NaN seen
    unsigned e1m = 0u, livem = 0u, seedm = 0u;
    unsigned negm[NS], nanm[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        negm[s] = nanm[s] = 0u;
    const size_t blk_rays = (size_t) n_rays;

    // the state that serves block m - 1: the -1 test, the exit ray (stored here), the bits; backward: the seed factors taken
    // at that state (Helper.h:518-529) into fs[]
    auto open_block = [&](const int mseg, double (&fs)[NS]) {
#define SPEC_SCAN_STATE
#define SPEC_SCAN_STATE_SEG mseg
#define SPEC_SCAN_STATE_F0 _Pragma("unroll") for (int s = 0; s < NS; s++) fs[s] = 0.0;
#define SPEC_SCAN_STATE_BITS                                                                                                   \
    if (!skip)                                                                                                                 \
        livem |= bit;                                                                                                          \
    if (!esc)                                                                                                                  \
        seedm |= bit;
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_STATE_BITS
#undef SPEC_SCAN_STATE_F0
#undef SPEC_SCAN_STATE_SEG
#undef SPEC_SCAN_STATE
        // (the seed factors last: nothing of the state but their four arguments is live across them; rt_spec_tile.inc)
        if (BACKWARD && have && !e1 && !esc) {
#define SPEC_TILE_FACTORS
#define SPEC_TILE_FS fs
#define SPEC_TILE_POINT const float px = spx, py = spy, pa = r2.a, pb = r2.b;
#include "rt_spec_tile.inc"
#undef SPEC_TILE_POINT
#undef SPEC_TILE_FS
#undef SPEC_TILE_FACTORS
        }
    };

    // ---- the stores and the walk, forward or backward: rt_spec_scan_seeds_walk.inc ----
#define SSS_WALK_TILE
#define SSS_OUT_IV Q->out.Iv
#include "rt_spec_scan_seeds_walk.inc"
#undef SSS_OUT_IV
#undef SSS_WALK_TILE

    // ---- the codes per seed (rt_spec_scan_tile.inc); a failing ray is reported once ----
    unsigned code = e1m ? 1u << 1 : 0u;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
#define SPEC_SCAN_CODES
#define SPEC_SCAN_CODES_CURVE s
#define SPEC_SCAN_CODES_NEG negm[s]
#define SPEC_SCAN_CODES_NAN nanm[s]
#define SPEC_SCAN_CODES_WORD H.ctl->seed_code[s]
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_CODES_WORD
#undef SPEC_SCAN_CODES_NAN
#undef SPEC_SCAN_CODES_NEG
#undef SPEC_SCAN_CODES_CURVE
#undef SPEC_SCAN_CODES
            code |= c;
        }
    }
    if (code)
        report_failure(code);
}

// The shell of rt_spec_kernel: one work-group of FREQ_WG_WAVES waves per CU, tiles from the eight sharded counters, one
// tile per fetch; LDS, all dynamic: the two exponent tables, then [64][XS_ROW] staging doubles per wave.
template <bool BACKWARD>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_spec_scan_seeds_kernel(const SpecScanSeedsKArg A)
{
    const int n_seed = A.set.n_seed;
#define SPEC_WG_KERNEL
#define SPEC_WG_KARG SpecScanSeedsKArg
#define SPEC_WG_BLOCK set
#define SPEC_WG_BLOCK_PTR SpecScanSeedsPtr
#define SPEC_WG_CALL spec_scan_seeds_tile<BACKWARD>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_CALL
#undef SPEC_WG_BLOCK_PTR
#undef SPEC_WG_BLOCK
#undef SPEC_WG_KARG
#undef SPEC_WG_KERNEL
}

} // namespace rt
