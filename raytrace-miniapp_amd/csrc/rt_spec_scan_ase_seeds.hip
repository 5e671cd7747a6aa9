#pragma once
// rt_spec_scan_ase_seeds.hip -- length spectra of an EMISSION plan that carries ASE seeds (rt_hip_plan_set_length_spectra_ase_seeds):
// RayTrace::calc_ray of the ASE problem AND of the same problem under up to RT_N_SEED_MAX seed beams, for every ray at every
// plasma length n = 2 .. N, from ONE scan march and ONE pass over the march record.
//
// The premises are those of rt_spec_scan.hip (the scan march leaves the state with which every ray crossed every length
// boundary; its table says which state serves row block n) and of rt_spec_ase_seeds.hip (the trajectory, gvl, the states and
// the escape flag do not depend on use_emis; only evl does).  rt_spec_scan_ase_seeds_kernel<BACKWARD> leaves (1 + n_seed) L
// row blocks, block r L + n - 2:
//   block (0, n)      the row rt_spec_scan_kernel<true, BACKWARD> leaves on this plan: its walk as text (rt_spec_scan_walk.inc)
//                     over the decode of rt_tile_rec.inc with its mask (true) and its live bits (F_SKIP: zeros), so the
//                     choice of the update is taken per slot as there; exact emission and the n = 3 rows of
//                     AseUpdate::apply_n3 included
//   block (1 + s, n)  the row rt_spec_scan_kernel<false, BACKWARD> leaves of the same problem created with seed s, i.e. block
//                     (s, n) of rt_spec_scan_seeds_kernel<BACKWARD>: its walk as text (rt_spec_scan_seeds_walk.inc), the
//                     association (f0_s sfk_s[k]) eg and the exponential-skip rule with `need` over all seeds
// It stands where rt_spec_scan_kernel stands, with the shell, LDS and grid of the single-seed pass (rt_spec_wg.inc).
//
// Per tile, once, the text of rt_spec_scan_tile.inc: the tile head and the record decode (SPEC_SCAN_HEAD, SPEC_SCAN_REC), and
// per block the state that serves it -- the -1 test, the exit ray (stored), the probe, one bit each for error -1, "has a row"
// and "not escaped" (open_state: SPEC_SCAN_STATE).  Then two halves over the frequencies, the HALVES of rt_spec_ase_seeds.hip:
//   emission half  spec_scan_tile<true, BACKWARD>'s walk, LSPEC_LCH = 4 lengths per staging, into blocks (0, .); the states
//                  are opened where that walk opens them (forward all ahead, backward chunk by chunk), each once
//   seed half      spec_scan_seeds_tile<BACKWARD>'s walk, SSS_LCH = 2 lengths x seeds per staging, into blocks (1 + s, .).
//                  The seed factors are taken at the head of this half -- forward once per ray at the launch ray (on a ray
//                  grid the product of the seed's tabulated factors), backward per chunk at the state that serves the block,
//                  read again from the boundary buffer -- so that nothing of them is live across the emission loop.
// The seed half reads the record and the lineshape rows again, from the caches.
// Registers: the backward seed walk fills the budget of 128 VGPRs by itself, so nothing is held across it that can be had
// again -- the ASE curve's codes are filed before it, the lane's numbers are formed anew at its head, error -1 comes back from
// the live bits, and the code of the ASE curve and the ray's number wait in the spare column of the lane's staging row.
// No scratch, no stack frame: 103 (forward) / 128 (backward) VGPRs, profiles/length_spectra_ase_seeds_kernel_resources.txt.
//
// F_SKIP: a ray whose every gvl / evl sum is zero gets rows of zeros in the ASE curve; under a seed it is live and carries
// f0_s f_s[4][k] exp(0) -- its zeroed and its real slots both give gl = +0 (rt_spec_ase_seeds.hip).
//
// Outputs, block-major then length-major in the one allocation of the mode: Iv [1 + n_seed][L][n_rays][K], err [1 + n_seed][L][n_rays],
// ray2 [L][n_rays].  Error -1 and the exit ray do not depend on r; -2 / -3 are per (r, n), -2 wins.  Every element is written.
// Failures: a ray is reported once with the OR of its codes over all (r, n); DevCtl::rec_code[r] carries the OR over n of
// curve r.  Nothing is deposited: no checking repeat.
#include "rt_spec_scan_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_spec.hip: the same contractions, the same doubles)

// the argument block is that of rt_spec_scan_seeds_kernel: out holds (1 + n_seed) L blocks here
template <bool BACKWARD>
__device__ __forceinline__ void spec_scan_ase_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SpecScanSeedsPtr Q, const int n_seed,
                                                         const double *tab, double *stage, const unsigned tile, int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int NS      = RT_N_SEED_MAX;

    // ---- the tile head of length spectra, once (rt_spec_scan_tile.inc; the lane's numbers are made opaque between the halves,
    // below); the march record of this lane's ray, the mask of spec_scan_tile ----
#define SPEC_SCAN_HEAD
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_HEAD
#define SPEC_SCAN_REC
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_REC

    // one bit per length (bit m - 1 = blocks (., n - 2)): error -1, the state gives rows (a ray, no error -1), not escaped
    // (carries the seed factors)
    unsigned e1m = 0u, okm = 0u, seedm = 0u;
    const size_t blk_rays = (size_t) n_rays;

    // the state that serves the blocks of m = mseg marched segments (the table of rt_spec_scan.hip), read where it is needed
    // as spec_scan_seeds_tile reads it: state_at; once per tile and length the -1 test, the exit ray (stored here), the
    // probe, the bits: open_state
#define SPEC_SCAN_STATE_AT
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_STATE_AT
    auto open_state = [&](const int mseg) {
#define SPEC_SCAN_STATE
#define SPEC_SCAN_STATE_SEG mseg
#define SPEC_SCAN_STATE_BY_LAMBDA
#define SPEC_SCAN_STATE_BITS                                                                                                  \
    okm |= bit;                                                                                                                \
    if (!esc)                                                                                                                  \
        seedm |= bit;
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_STATE_BITS
#undef SPEC_SCAN_STATE_BY_LAMBDA
#undef SPEC_SCAN_STATE_SEG
#undef SPEC_SCAN_STATE
    };

    // The codes of curve r from its bits (rt_spec_scan_tile.inc), filed as soon as the half that leaves the curve is through,
    // so that no bit of the ASE curve is held across the seed half; returns the code of the curve for this ray
    auto file_codes = [&](const int r, const unsigned e1m, const unsigned negm, const unsigned nanm) -> unsigned {
#define SPEC_SCAN_CODES
#define SPEC_SCAN_CODES_CURVE r
#define SPEC_SCAN_CODES_NEG negm
#define SPEC_SCAN_CODES_NAN nanm
#define SPEC_SCAN_CODES_WORD H.ctl->rec_code[r]
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_CODES_WORD
#undef SPEC_SCAN_CODES_NAN
#undef SPEC_SCAN_CODES_NEG
#undef SPEC_SCAN_CODES_CURVE
#undef SPEC_SCAN_CODES
        return c;
    };
    unsigned code = 0u; // the OR over all (r, n): a failing ray is reported once

    // ================= the emission half: blocks (0, .), the walk of spec_scan_tile<true, BACKWARD> =================
    {
        constexpr bool EMIS      = true;
        constexpr int LCH        = LSPEC_LCH;
        constexpr double f0_launch = 0.0; // (the gain-only half of the walk's text is dead here: what it names)
        const ConstF64 sfk       = (ConstF64) (unsigned long long) H.seed_fk;
        unsigned livem = 0u, negm = 0u, nanm = 0u;
        // the walk opens every state once, where spec_scan_tile opens it; a row of the ASE curve is live unless F_SKIP
        auto open_block = [&](const int mseg) -> double {
            open_state(mseg);
            livem = skip ? 0u : okm;
            return 0.0;
        };
#include "rt_spec_scan_walk.inc"
        code = file_codes(0, e1m, negm, nanm);
    }

    // ================= the seed half: blocks (1 + s, .), the walk of spec_scan_seeds_tile<BACKWARD> =================
    {
        constexpr int LCH = SSS_LCH;
        // (the lane's numbers and the bits opaque at the head of this half: what the emission half derived of them -- staging
        // and record addresses -- is not kept for this one, which forms its own)
        asm volatile("" : "+v"(lane));
        ridx = row0 + (unsigned) lane;
        rrec = have ? ridx : 0u;
        // (what the end of the tile wants back and the walk does not read -- the code of the ASE curve, the ray's number for
        // the codes and the report -- waits in the spare column of the lane's own staging row, which no flush reads: the
        // backward instance has no register to spare for them, and no scratch; profiles/length_spectra_ase_seeds_kernel_resources.txt)
        static_assert(SSS_LCH * RT_N_SEED_MAX * VEC + 1 <= XS_ROW && LSPEC_LCH * VEC + 1 <= XS_ROW, "a staging row has a spare column behind the staged values");
        unsigned *spare = reinterpret_cast<unsigned *>(stage + lane * XS_ROW + (XS_ROW - 1));
        spare[0]        = code;
        spare[1]        = ridx;
        // (every length of a lane that holds a ray has either bit: e1m is not held across this half, it comes back from livem)
        unsigned livem = okm;
        asm volatile("" : "+v"(livem), "+v"(seedm));
        // the seed factors at the launch ray (forward)
        // (an emission plan has no creation seed and hence no R.sf: the seeds' tables are there where they serve the run, rt_launch.hip)
#define SSS_WALK_F0
#define SSS_GRID_TABS Q->tabs.sf[0]
#include "rt_spec_scan_seeds_walk.inc"
#undef SSS_GRID_TABS
#undef SSS_WALK_F0
        unsigned negm[NS], nanm[NS];
#pragma unroll
        for (int s = 0; s < NS; s++)
            negm[s] = nanm[s] = 0u;
        // the states are open; backward the seed factors of a block are taken at its state (Helper.h:518-529), read again
        auto open_block = [&](const int mseg, double (&fs)[NS]) {
#pragma unroll
            for (int s = 0; s < NS; s++)
                fs[s] = 0.0;
            if (BACKWARD && ((seedm >> (mseg - 1)) & 1u) != 0u) { // (a ray, no error -1, not escaped)
                const float *q  = state_at(mseg);
                const float spx = q[0], spy = q[1], ssx = q[2], ssy = q[3], ssz = q[4];
                const float ra = atanf_flt32_kernel(ssx / ssz) * 1e3f, rb = atanf_flt32_kernel(ssy / ssz) * 1e3f;
#define SPEC_TILE_FACTORS
#define SPEC_TILE_FS fs
#define SPEC_TILE_POINT const float px = spx, py = spy, pa = ra, pb = rb;
#include "rt_spec_tile.inc"
#undef SPEC_TILE_POINT
#undef SPEC_TILE_FS
#undef SPEC_TILE_FACTORS
            }
        };
#define SSS_WALK_TILE
#define SSS_OUT_IV (Q->out.Iv + (size_t) L * blk_rays * (size_t) K)
#include "rt_spec_scan_seeds_walk.inc"
#undef SSS_OUT_IV
#undef SSS_WALK_TILE
        code = spare[0];
        ridx = spare[1];
        const unsigned e1s = have ? ~livem & (L >= 32 ? ~0u : (1u << L) - 1u) : 0u;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (s < n_seed)
                code |= file_codes(1 + s, e1s, negm[s], nanm[s]);
        }
    }

    if (code)
        report_failure(code);
}

// The shell of rt_spec_kernel: one work-group of FREQ_WG_WAVES waves per CU, tiles from the eight sharded counters, one
// tile per fetch; LDS, all dynamic: the two exponent tables, then [64][XS_ROW] staging doubles per wave.  The register budget
// of rt_spec_scan_kernel<true, BACKWARD>.
template <bool BACKWARD>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES) rt_spec_scan_ase_seeds_kernel(const SpecScanSeedsKArg A)
{
    const int n_seed = A.set.n_seed;
#define SPEC_WG_KERNEL
#define SPEC_WG_KARG SpecScanSeedsKArg
#define SPEC_WG_BLOCK set
#define SPEC_WG_BLOCK_PTR SpecScanSeedsPtr
#define SPEC_WG_CALL spec_scan_ase_seeds_tile<BACKWARD>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_CALL
#undef SPEC_WG_BLOCK_PTR
#undef SPEC_WG_BLOCK
#undef SPEC_WG_KARG
#undef SPEC_WG_KERNEL
}

} // namespace rt
