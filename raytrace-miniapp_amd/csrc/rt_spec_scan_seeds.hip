#pragma once
// rt_spec_scan_seeds.hip -- length spectra with the seeds of rt_hip_plan_set_spectra_seeds: RayTrace::calc_ray for every ray
// at every plasma length n = 2 .. N under up to RT_N_SEED_MAX seed beams, from ONE scan march and ONE walk over the record.
//
// The premises are those of rt_spec_scan.hip and rt_step_scan_seeds.hip / rt_step_rscan_seeds.hip: the scan march leaves the
// state with which every ray crossed every length boundary, the table of rt_spec_scan.hip says which state serves row block
// n, and neither the march record nor those states hold anything of the seed, which enters as
// Iv_{s,n}[k] = (f0_{s,n} f_s[4][k]) exp(gl_n[k]) only.  rt_spec_scan_seeds_kernel<BACKWARD> stands where
// rt_spec_scan_kernel<false, BACKWARD> stands, gain-only, with its shell, LDS and launch bounds.
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
    const int L           = H.L;
    const int S           = L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned row0   = tile * WAVE;
    const unsigned ridx   = row0 + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = BACKWARD;
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;

    // ---- per-ray preamble, once: the final state of the ray (rt_tile_ray.inc) ----
#define TILE_NEED_RAY false
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    (void) err1; // (of the final state: every block takes the test of its own state, open_block)
    if (__ballot(have) == 0ull)
        return;
    // the marched segment the ray escaped in (never: L + 1)
    const int n_done           = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
    const unsigned flags_steps = m.flags_steps;
    const int e_seg            = (fl & F_ESCAPED) ? (n_done > 0 ? (n_done - 1) / RT_N_SUB + 1 : 1) : L + 1;
    const bool skip            = (fl & F_SKIP) != 0u; // every update is the identity: rows of zeros at every n

#define SSS_WALK_F0
#define SSS_GRID_TABS R.sf
#include "rt_spec_scan_seeds_walk.inc"
#undef SSS_GRID_TABS
#undef SSS_WALK_F0

    // ---- the march record of this lane's ray (rt_tile_rec.inc; SF = 0: nothing to decode up front) ----
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
    (void) gs;
    (void) rs;
    (void) off;
    (void) all_small;
    (void) all_regular;
    (void) load_rows;
    (void) gv_nan;
    (void) exact_emis;

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
        // a boundary state or the final one, which begin with the same five floats (position, direction) -- read where it is
        // needed, so that no state is held across the seed factors (rt_step_rscan_seeds.hip)
        static_assert(offsetof(RecMeta, px) == 0 && offsetof(RecMeta, sz) == 16, "a boundary state and a RecMeta begin alike");
        const bool at_bnd = mseg < L && mseg < e_seg;
        const bool esc    = !at_bnd && (fl & F_ESCAPED) != 0u;
        float spx = 0.0f, spy = 0.0f, ssx = 0.0f, ssy = 0.0f, ssz = 1.0f;
        if (have) {
            const float *q = reinterpret_cast<const float *>(at_bnd ? Q->bnd + scan_bnd_off(ridx, mseg, L) : rec + rec_meta_off(rrec, S, H.rec_stride));
            spx            = q[0];
            spy            = q[1];
            ssx            = q[2];
            ssy            = q[3];
            ssz            = q[4];
        }
        const unsigned bit = 1u << (mseg - 1);
        const bool e1      = have && (double) (ssz * ssz) < 0.01; // Helper.h:515
        rt_ray r2          = { 0.0f, 0.0f, 0.0f, 0.0f };          // (zeros under error -1, as rt_spec.hip leaves them)
#pragma unroll
        for (int s = 0; s < NS; s++)
            fs[s] = 0.0;
        if (have && !e1) {
            r2.x = spx; // Helper.h:518-521
            r2.y = spy;
            r2.a = atanf_flt32_kernel(ssx / ssz) * 1e3f;
            r2.b = atanf_flt32_kernel(ssy / ssz) * 1e3f;
            if (!skip)
                livem |= bit;
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
        // (the seed factors last: nothing of the state but their four arguments is live across them)
        if (BACKWARD && have && !e1 && !esc) {
#pragma unroll 1
            for (int s = 0; s < n_seed; s++) {
                const double f = rscan_seed_factor(&Q->tabs.seed[s], (double) spx, (double) spy, (double) r2.a, (double) r2.b);
#pragma unroll
                for (int t = 0; t < NS; t++)
                    fs[t] = t == s ? f : fs[t];
            }
        }
    };

    // ---- the stores and the walk, forward or backward: rt_spec_scan_seeds_walk.inc ----
#define SSS_WALK_TILE
#define SSS_OUT_IV Q->out.Iv
#include "rt_spec_scan_seeds_walk.inc"
#undef SSS_OUT_IV
#undef SSS_WALK_TILE

    // ---- the codes per seed: -1 of the state, else -2 over -3 (Helper.h:588-593: negative wins); a failing ray is reported once ----
    unsigned code = e1m ? 1u << 1 : 0u;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            if (have) {
#pragma unroll 1
                for (int jb = 0; jb < L; jb++) {
                    const unsigned bit = 1u << jb;
                    Q->out.err[((size_t) s * (size_t) L + (size_t) jb) * blk_rays + ridx] =
                        (e1m & bit) ? -1 : ((negm[s] & bit) ? -2 : ((nanm[s] & bit) ? -3 : 0));
                }
            }
            const unsigned only_nan = nanm[s] & ~negm[s];
            const unsigned c        = (e1m ? 1u << 1 : 0u) | (negm[s] ? 1u << 2 : 0u) | (only_nan ? 1u << 3 : 0u);
            if (c)
                atomicOr(&H.ctl->seed_code[s], c);
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
    // per tile: the cold half and the seeds of the argument block, the flag word and the lane number opaque
#define SPEC_WG_KERNEL
#define SPEC_WG_TILE                                                                                                    \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecScanSeedsKArg, cold)); \
    SpecScanSeedsPtr Q = (SpecScanSeedsPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecScanSeedsKArg, set)); \
    asm volatile("" : "+s"(C), "+s"(Q)); \
    unsigned hflags = H.flags; \
    int lane_t      = lane; \
    asm volatile("" : "+s"(hflags), "+v"(lane_t)); \
    spec_scan_seeds_tile<BACKWARD>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_TILE
#undef SPEC_WG_KERNEL
}

} // namespace rt
