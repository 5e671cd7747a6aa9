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
// Per tile, once: the preamble (rt_tile_ray.inc), the record decode, and per block the state that serves it -- the -1 test,
// the exit ray (stored), the probe, one bit each for error -1, "has a row" and "not escaped" (open_state).  Then two halves
// over the frequencies, the HALVES of rt_spec_ase_seeds.hip:
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
    const int L           = H.L;
    const int S           = L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned row0   = tile * WAVE;
    unsigned ridx         = row0 + (unsigned) lane; // (the lane's numbers are made opaque between the halves, below)
    const bool have       = ridx < n_rays;
    const bool backward   = BACKWARD;
    unsigned rrec            = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;

    // ---- per-ray preamble, once: the final state of the ray (rt_tile_ray.inc) ----
#define TILE_NEED_RAY false
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    (void) err1; // (of the final state: every block takes the test of its own state, open_state)
    if (__ballot(have) == 0ull)
        return;
    // the marched segment the ray escaped in (never: L + 1)
    const int n_done           = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
    const unsigned flags_steps = m.flags_steps;
    const int e_seg            = (fl & F_ESCAPED) ? (n_done > 0 ? (n_done - 1) / RT_N_SUB + 1 : 1) : L + 1;
    const bool skip            = (fl & F_SKIP) != 0u; // every update is the identity: zeros in the ASE curve at every n

    // ---- the march record of this lane's ray (rt_tile_rec.inc; SF = 0: nothing to decode up front), the mask of spec_scan_tile ----
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
    (void) gs;
    (void) rs;
    (void) off;
    (void) all_small;
    (void) all_regular;
    (void) load_rows;
    (void) gv_nan; // (SF = 0 tests every frequency's lineshape values as it reads them)

    // one bit per length (bit m - 1 = blocks (., n - 2)): error -1, the state gives rows (a ray, no error -1), not escaped
    // (carries the seed factors)
    unsigned e1m = 0u, okm = 0u, seedm = 0u;
    const size_t blk_rays = (size_t) n_rays;
    static_assert(offsetof(RecMeta, px) == 0 && offsetof(RecMeta, sz) == 16, "a boundary state and a RecMeta begin alike");

    // the state that serves the blocks of m = mseg marched segments (the table of rt_spec_scan.hip): a boundary state or the
    // final one, read where it is needed as spec_scan_seeds_tile reads it
    auto state_at = [&](const int mseg) -> const float * {
        const bool at_bnd = mseg < L && mseg < e_seg;
        return reinterpret_cast<const float *>(at_bnd ? Q->bnd + scan_bnd_off(ridx, mseg, L) : rec + rec_meta_off(rrec, S, H.rec_stride));
    };
    // ... once per tile and length: the -1 test, the exit ray (stored here), the probe, the bits
    auto open_state = [&](const int mseg) {
        const bool esc = !(mseg < L && mseg < e_seg) && (fl & F_ESCAPED) != 0u;
        float spx = 0.0f, spy = 0.0f, ssx = 0.0f, ssy = 0.0f, ssz = 1.0f;
        if (have) {
            const float *q = state_at(mseg);
            spx            = q[0];
            spy            = q[1];
            ssx            = q[2];
            ssy            = q[3];
            ssz            = q[4];
        }
        const unsigned bit = 1u << (mseg - 1);
        const bool e1      = have && (double) (ssz * ssz) < 0.01; // Helper.h:515
        rt_ray r2          = { 0.0f, 0.0f, 0.0f, 0.0f };          // (zeros under error -1, as rt_spec.hip leaves them)
        if (have && !e1) {
            r2.x = spx; // Helper.h:518-521
            r2.y = spy;
            r2.a = atanf_flt32_kernel(ssx / ssz) * 1e3f;
            r2.b = atanf_flt32_kernel(ssy / ssz) * 1e3f;
            okm |= bit;
            if (!esc)
                seedm |= bit;
        }
        if (e1)
            e1m |= bit;
        if (have) {
            Q->out.ray2[(size_t) (mseg - 1) * blk_rays + ridx] = r2;
            if (probe_on && mseg == L) { // the probe is that of the whole run
                C->probe.ray2[ridx]  = r2;
                C->probe.flags[ridx] = fl | (e1 ? F_ERR1 : 0u);
                C->probe.steps[ridx] = steps;
            }
        }
    };

    // The codes of curve r from its bits (a negative value seen, a NaN seen; one bit per length), filed as soon as the half
    // that leaves the curve is through, so that no bit of the ASE curve is held across the seed half: per (r, n) -1 of the
    // state, else -2 over -3 (Helper.h:588-593: negative wins); returns the code of the curve for this ray
    auto file_codes = [&](const int r, const unsigned e1m, const unsigned negm, const unsigned nanm) -> unsigned {
        if (have) {
#pragma unroll 1
            for (int jb = 0; jb < L; jb++) {
                const unsigned bit = 1u << jb;
                Q->out.err[((size_t) r * (size_t) L + (size_t) jb) * blk_rays + ridx] = (e1m & bit) ? -1 : ((negm & bit) ? -2 : ((nanm & bit) ? -3 : 0));
            }
        }
        const unsigned only_nan = nanm & ~negm;
        const unsigned c        = (e1m ? 1u << 1 : 0u) | (negm ? 1u << 2 : 0u) | (only_nan ? 1u << 3 : 0u);
        if (c)
            atomicOr(&H.ctl->rec_code[r], c);
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
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double f = rscan_seed_factor(&Q->tabs.seed[s], (double) spx, (double) spy, (double) ra, (double) rb);
#pragma unroll
                    for (int t = 0; t < NS; t++)
                        fs[t] = t == s ? f : fs[t];
                }
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
    // per tile: the cold half and the seeds of the argument block, the flag word and the lane number opaque
#define SPEC_WG_KERNEL
#define SPEC_WG_TILE                                                                                                    \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecScanSeedsKArg, cold)); \
    SpecScanSeedsPtr Q = (SpecScanSeedsPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecScanSeedsKArg, set)); \
    asm volatile("" : "+s"(C), "+s"(Q)); \
    unsigned hflags = H.flags; \
    int lane_t      = lane; \
    asm volatile("" : "+s"(hflags), "+v"(lane_t)); \
    spec_scan_ase_seeds_tile<BACKWARD>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_TILE
#undef SPEC_WG_KERNEL
}

} // namespace rt
