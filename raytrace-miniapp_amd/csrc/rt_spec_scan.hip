#pragma once
// rt_spec_scan.hip -- length spectra (rt_hip_plan_enable_length_spectra): RayTrace::calc_ray for every ray at every
// plasma length n = 2 .. N from ONE march.
//
// The scan instance of the march (rt_march.hip, MARCH_OPT_SCAN) runs unchanged and leaves the state with which every ray
// crossed every length boundary.  With the forward method the sub-problem of n lengths is problem.prefix_lengths: the first
// 3 (n - 1) slots of the march record (rt_step_scan.hip); with the backward method it is problem.suffix_lengths: the last
// 3 (n - 1) slots (rt_step_rscan.hip).  Which state serves row block n (m = n - 1 marched segments, L = N - 1; e = the
// marched segment the ray escaped in, L + 1 if never) is the table of those two files:
//   not escaped, m < L      boundary m                          not escaped, m = L      the final RecMeta
//   escaped,     m < e      boundary m, the ray NOT escaped     escaped,     m >= e     the final RecMeta, escaped
// Error -1 of block n is s.z^2 < 0.01 of that state, ray2 its position and exit angles (atanf_flt32_kernel), the seed
// factor (gain-only mode) is taken at the launch ray (forward) or at that state (backward) and is 0 once the ray has
// escaped.  Rows follow rt_spec.hip: error -1 and a ray whose every update is the identity give a row of zeros, -2 wins
// over -3.
//
// rt_spec_scan_kernel<EMIS, BACKWARD> stands where rt_spec_kernel stands and has its shell: one 16-wave work-group per CU,
// tiles from the eight sharded counters, lanes = rays, the LDS of rt_spec_kernel (the exponent tables and [64][XS_ROW]
// staging doubles per wave), its launch bounds.  The tile text is that of the scan kernels: rt_tile_ray.inc, rt_tile_rec.inc
// with SF = 0, rec_slot_lazy, so the arithmetic of a slot is rt_tile_batch.inc's for SF = 0.  The tile head, the state that
// serves a block and the codes of a curve are the text the three tile functions of length spectra share
// (rt_spec_scan_tile.inc), the walk and its stores that of rt_spec_scan_walk.inc.
//   forward   the prefixes share one running spectrum: per frequency batch ONE walk over the slots, and the running Iv
//             (gain-only: one exp_tab_vec of the running gl) after the three sub-segments of length j is row n = j + 1.
//   backward  suffix n starts with its own initial value at slot 3 (N - n): the walk of rt_step_rscan.hip, LSPEC_LCH
//             accumulators per walk that join one segment after the other, e^gl - 1 of a slot taken once (ase_factor),
//             irregular sub-segments and the exact mode through ase_update_factors; gain-only one f64 product sum per suffix.
// In gain-only mode and with exact emission every Iv_n[k] is the double rt_spec_kernel computes on the sub-problem.  (The plan
// of the N = 3 sub-problem takes rt_spec_kernel<6, true>, which contracts the last line of ase_update otherwise than
// rt_spec_kernel<0, true>: with exact emission the rows of n = 3 are integrated in that form, AseUpdate::apply_n3 -- forward by a
// second running spectrum over the first six slots, backward in the accumulator of that suffix)  In the
// default emission mode the sub-problem's plan may take another update (its tile-wide choice sees other slots, and its
// N = 3 instance has SF = 6), as the records of the scan kernels differ from a step plan's.
//
// Outputs, length-major: Iv [L][n_rays][K] (row stride K), ray2 [L][n_rays], err [L][n_rays]; block n - 2 has the shape
// of spectra mode's output of the sub-problem.  Every element is written.
//
// The stores.  A wave cannot hold L stagings of 16 frequencies, so the staging rows are cut the other way: VEC frequencies
// of LSPEC_LCH = 4 lengths per lane ([64][XS_ROW], column li * VEC + v).  When four lengths are staged (forward: every
// fourth length of the walk; backward: the end of a chunk's walk) each length leaves as 64 row pieces of 32 bytes, 16 bytes
// per lane and 32 rows per instruction; the next frequency batches complete the cache lines in L2, as rt_spec.hip found
// ordinary stores do.  No slot is integrated twice for the stores' sake.  Ragged last tiles and odd K keep rt_spec.hip's
// 8-byte path; a last batch of two frequencies (K = 4 i + 2) leaves as one 16-byte piece per row.
#include "rt_spec.hip"
#include "rt_step_rscan.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_spec.hip: the same contractions, the same doubles)

constexpr int LSPEC_LCH = 4; // lengths per staging: LSPEC_LCH * VEC doubles of a staging row
static_assert(LSPEC_LCH * VEC <= XS_ROW - 2 && VEC == 4, "a staging row holds VEC frequencies of LSPEC_LCH lengths");

// what rt_spec_scan_kernel reads beside the frequency kernel's block (through the constant address space, as the cold half)
struct SpecScanArg {
    SpecOut out;              // Iv [L][n_rays][K], ray2 [L][n_rays], err [L][n_rays]
    const unsigned char *bnd; // boundary states of the march (scan_bnd_off)
};
struct SpecScanKArg {
    FreqHot hot;
    FreqCold cold;
    SpecScanArg scan;
};
typedef const RT_CONST_AS SpecScanArg *SpecScanPtr;

// ase_update (rt_freq.hip) for several accumulators of one (sub-segment, frequency): what of the update does not depend on Iv
// is taken once -- small |gl|: Iv' = el X + Iv B, else Iv' = (el / gl) (e^gl - 1) + Iv e^gl -- and apply() finishes it per
// accumulator.  The roundings are written out as the compiler contracts ase_update where it stands alone (ase_update_call,
// rt_step_rscan.hip): fma(X, el, Iv B) and fma(Iv, e^gl, t).  (That call itself is not taken here: with one more caller of it,
// or with another function held to a call beside it, rt_step_rscan_kernel<true> and rt_step_rscan_ase_seeds_kernel came out of
// the compiler with other registers; ase_update inlined per accumulator and frequency left the backward emission instance 176
// bytes of scratch.  profiles/length_spectra_kernel_resources.txt)
struct AseUpdate {
    double a, b, c; // small |gl|: X, B, el; else: t = (el / gl) (e^gl - 1), e^gl, unused
    bool small;
    __device__ __forceinline__ double apply(const double Iv) const { return small ? fma(a, c, Iv * b) : fma(Iv, b, a); }
    // ... as rt_spec_kernel<6, true> contracts it, the instance a spectra-mode plan of an N = 3 problem takes: there the two
    // branches meet behind the product that does not hold Iv, so the small branch is fma(Iv, B, el X) as well (read from
    // its device assembly: 24 of 24 updates; the other branch is the same in both instances).  With exact emission the rows
    // of n = 3 take this form, so that they are the doubles of that plan (measured otherwise: one unit in the last place
    // in 4 % of the values).  This restates by hand what the compiler made of ase_update inside ANOTHER kernel: it holds for
    // that code object and no longer.  A compiler update, or an edit of rt_spec.hip, rt_tile_batch.inc or rt_freq.hip, may move
    // the contraction there without a word, and only tests/test_gpu_length_spectra.py (exact emission, n = 3) would notice;
    // writing the form out in rt_spec_kernel<6> as well, so that both sides are explicit, is left to a change that may
    // touch that kernel.
    __device__ __forceinline__ double apply_n3(const double Iv) const { return fma(Iv, b, small ? a * c : a); }
};
__device__ __forceinline__ AseUpdate ase_update_factors(const float gs, const float es, const float w, const double *tab)
{
    const double gl = (double) (gs * w); // f32 product, then widened (Helper.h:549-550)
    const double el = (double) (es * w);
    AseUpdate u;
    u.small = fabs(gl) < 1e-3;
    if (u.small) {
        u.a = fma(0.5 * gl, fma(gl, 0.3333333333, 1.0), 1.0);
        u.b = fma(fma(gl, 0.5, 1.0), gl, 1.0);
        u.c = el;
    } else {
        const double eg = exp_tab(gl, tab);
        u.a             = div_fast(el, gl) * (eg - 1.0);
        u.b             = eg;
        u.c             = 0.0;
    }
    return u;
}

template <bool EMIS, bool BACKWARD>
__device__ __forceinline__ void spec_scan_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SpecScanPtr Q, const double *tab, double *stage,
                                               const unsigned tile, const int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH     = LSPEC_LCH;
    const bool seeded     = !EMIS && (hflags & FQ_HAS_SEED) != 0; // (the emission recurrence takes no seed factor)

    // ---- the tile head of length spectra, once: the final state of the ray, the segment it escaped in (rt_spec_scan_tile.inc) ----
#define SPEC_SCAN_HEAD
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_HEAD

    // the seed factor at the launch ray (forward, Helper.h:530-533), in place_ray's own arithmetic as rt_step_scan.hip takes it
    double f0_launch = 0.0;
    if (!BACKWARD && have && seeded) {
        if (!R.sf) {
            rt_ray launch = ray;
            float ta, tb;
            load_ray(R, ridx, launch, ta, tb, false);
            // (rscan_seed_factor: scan_seed_factor on a seed that stays in the argument block -- with the copy this instance kept
            // a 48-byte stack frame that nothing read)
            f0_launch = rscan_seed_factor(&C->seed, (double) launch.x, (double) launch.y, (double) launch.a, (double) launch.b);
        } else {
            RT_SEED_GRID_POINT(R, ridx)
            RT_SEED_GRID_FACTOR(f0_launch, C->seed.f0, R.sf, R.sin)
        }
    }

    // ---- the march record of this lane's ray (rt_tile_rec.inc; SF = 0: nothing to decode up front) ----
#define SPEC_SCAN_REC
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_REC
    const ConstF64 sfk = (ConstF64) (unsigned long long) H.seed_fk;

    // one bit per row block (bit m - 1 = block n - 2): error -1, live, not escaped (carries the seed factor), a negative
    // value seen, a NaN seen
    unsigned e1m = 0u, livem = 0u, seedm = 0u, negm = 0u, nanm = 0u;
    const size_t blk_rays = (size_t) n_rays;

    // the state that serves block m - 1: the -1 test, the exit ray (stored here), the bits; returns the seed factor of the
    // backward method, taken at that state (Helper.h:518-529)
    auto open_block = [&](const int mseg) -> double {
#define SPEC_SCAN_STATE
#define SPEC_SCAN_STATE_SEG mseg
#define SPEC_SCAN_STATE_HELD
#define SPEC_SCAN_STATE_F0 double f0 = 0.0;
#define SPEC_SCAN_STATE_BITS                                                                                                   \
    if (!skip)                                                                                                                 \
        livem |= bit;                                                                                                          \
    if (seeded && !esc) {                                                                                                      \
        seedm |= bit;                                                                                                          \
        if (BACKWARD)                                                                                                          \
            f0 = rscan_seed_factor(&C->seed, (double) spx, (double) spy, (double) r2.a, (double) r2.b);                        \
    }
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_STATE_BITS
#undef SPEC_SCAN_STATE_F0
#undef SPEC_SCAN_STATE_HELD
#undef SPEC_SCAN_STATE_SEG
#undef SPEC_SCAN_STATE
        return f0;
    };

    // ---- the stores and the walk, forward or backward: rt_spec_scan_walk.inc ----
#include "rt_spec_scan_walk.inc"

    // ---- the codes (rt_spec_scan_tile.inc: no code word beside the ray's); a failing ray is reported once ----
#define SPEC_SCAN_CODES
#define SPEC_SCAN_CODES_CURVE 0
#define SPEC_SCAN_CODES_NEG negm
#define SPEC_SCAN_CODES_NAN nanm
#include "rt_spec_scan_tile.inc"
#undef SPEC_SCAN_CODES_NAN
#undef SPEC_SCAN_CODES_NEG
#undef SPEC_SCAN_CODES_CURVE
#undef SPEC_SCAN_CODES
    if (c)
        report_failure(c);
}

// The shell of rt_spec_kernel: one work-group of FREQ_WG_WAVES waves per CU, tiles from the eight sharded counters, one
// tile per fetch; LDS, all dynamic: the two exponent tables, then [64][XS_ROW] staging doubles per wave.
template <bool EMIS, bool BACKWARD>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_spec_scan_kernel(const SpecScanKArg A)
{
#define SPEC_WG_KERNEL
#define SPEC_WG_KARG SpecScanKArg
#define SPEC_WG_BLOCK scan
#define SPEC_WG_BLOCK_PTR SpecScanPtr
#define SPEC_WG_CALL spec_scan_tile<EMIS, BACKWARD>(H, hflags, C, Q, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_CALL
#undef SPEC_WG_BLOCK_PTR
#undef SPEC_WG_BLOCK
#undef SPEC_WG_KARG
#undef SPEC_WG_KERNEL
}

} // namespace rt
