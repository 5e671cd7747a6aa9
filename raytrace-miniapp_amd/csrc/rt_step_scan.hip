#pragma once
// rt_step_scan.hip -- step mode with a length scan (rt_hip_plan_enable_length_scan): the step record at every plasma
// length n = 2 .. N from ONE forward march.
//
// With the forward method RayTrace_calc_ray walks the lengths ii = 1, 2, ... in order (Helper.h:430-441): its run with n
// lengths is the first n - 1 iterations of the outer loop of its run with N lengths, so the first 3 (n - 1) slots of the
// march record (gvl / evl / ivl) of the N-run are the whole record of the n-run.  What the n-run has and the N-run's record
// has not is the state with which the ray LEFT length j = n - 1: the scan instance of the march (rt_march.hip,
// MARCH_OPT_SCAN) stores it where the ray crosses the boundary.  Which state serves length j, and error -1 under it:
// rt_step_scan_state.inc.  The seed factor is taken at the launch ray (Helper.h:530-533) and is 0 where the ray has
// escaped by j.
//
// rt_step_scan_kernel stands where rt_step_kernel stands and has its shape: the shell of the scan passes
// (rt_step_scan_wg.inc), the tile preamble they share (rt_step_scan_tile.inc), the forward walk (rt_step_scan_walk.inc: the
// arithmetic of a slot, why every Iv_j[k] is the double rt_step_kernel<0, EMIS> computes on the prefix problem) and the
// close of a record (rt_step_scan_close.inc).  (The tile-wide choice between ase_step_f32 / ase_step / ase_update exists in
// the SF = 6 instances only: with a run-time number of slots the choice is per slot, and a prefix of the slots takes the
// choices of the whole.)
//
// Per tile the lengths are taken in chunks of SCAN_LCH, unrolled under the wave-uniform test j <= L as the seed loops of
// rt_step_seeds.hip are: what is live per lane and length -- pixel, angle cell, the sum over k, and one bit each for "live",
// "carries the seed factor" and "a negative Iv seen" -- stays in registers with compile-time indices.  Chunk c integrates
// the 3 LCH (c - 1) slots below it again; at the end of the chunk, per length, the runs of equal pixel AT THAT LENGTH
// (rt_wave_runs.inc), the failure test, the I_ang add and the segmented nf scan.
//
// Failures follow the reference run once per length: error -1 at length j sets bit 1 of that length's code and keeps the
// ray out of record j; error -2 / -3 at length j removes the ray from record j only.  A ray that fails at any length is
// reported once, with the OR of its codes; DevCtl::len_code[j - 1] holds the code of length j.  The checking repeat keeps
// its two passes; the mark of a ray is one bit per length in a 32-bit word (FreqHot::bad is an array of words here),
// written by the one lane that holds the ray.
#include "rt_step_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int SCAN_LCH = 4; // lengths per pass over a tile

// what rt_step_scan_kernel reads beside the frequency kernel's block (through the constant address space, as the cold half)
struct ScanArg {
    const unsigned char *bnd; // boundary states of the march (scan_bnd_off)
    double *out;              // L blocks of `stride` doubles: E_v | nf at nf_off | I_ang at ang_off
    unsigned long long stride, nf_off, ang_off;
};
struct ScanKArg {
    FreqHot hot;
    FreqCold cold;
    ScanArg scan;
};
typedef const RT_CONST_AS ScanArg *ScanPtr;

// seed_factor (rt_math.h), statement by statement, with pchip_eval held to a call as the other kernels have it: inlined
// four times into this kernel it left the gain-only instance a 48-byte stack frame (that nothing read)
__device__ __forceinline__ double scan_seed_factor(const DevSeed &sd, double x, double y, double a, double b)
{
    double f = 0.0;
    if (x >= sd.x[0][0] && x <= sd.x[0][sd.dim[0] - 1] && y >= sd.x[1][0] && y <= sd.x[1][sd.dim[1] - 1] &&
        a >= sd.x[2][0] && a <= sd.x[2][sd.dim[2] - 1] && b >= sd.x[3][0] && b <= sd.x[3][sd.dim[3] - 1]) {
        double fx, fy, fa, fb;
        [[clang::noinline]] fx = pchip_eval(sd.dim[0], sd.x[0], sd.f[0], x);
        [[clang::noinline]] fy = pchip_eval(sd.dim[1], sd.x[1], sd.f[1], y);
        [[clang::noinline]] fa = pchip_eval(sd.dim[2], sd.x[2], sd.f[2], a);
        [[clang::noinline]] fb = pchip_eval(sd.dim[3], sd.x[3], sd.f[3], b);
        f = sd.f0 * fx * fy * fa * fb;
        f = f < 0.0 ? 0.0 : f;
    }
    return f;
}

template <bool EMIS>
__device__ __forceinline__ void step_scan_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, double *lds_iang, double *lds_ev,
                                               const double *tab, double *xpose, const unsigned tile, const int lane)
{
    constexpr int SF  = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH = SCAN_LCH;
#define SCAN_TILE_BACKWARD false // the forward method: rt_hip_plan_enable_length_scan takes no other
#define SCAN_TILE_MARK unsigned
#define SCAN_TILE_HEAD
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_HEAD
#undef SCAN_TILE_BACKWARD
#undef SCAN_TILE_MARK
    // the seed factor at the launch ray, in place_ray's own arithmetic (it does not depend on the exit state with the
    // forward method); 0 without a seed
    double f0_launch = 0.0;
    if (have && (hflags & FQ_HAS_SEED)) { // place_ray's seed half for the forward method (Helper.h:523-533), its arithmetic and order
        if (!R.sf) {
            rt_ray launch = ray;
            float ta, tb;
            load_ray(R, ridx, launch, ta, tb, false);
            const DevSeed SD = load_cold(&C->seed);
            f0_launch        = scan_seed_factor(SD, (double) launch.x, (double) launch.y, (double) launch.a, (double) launch.b);
        } else {
            // the launch ray is a grid point: product of the tabulated factors (RT_SEED_GRID_FACTOR)
            RT_SEED_GRID_POINT(R, ridx)
            RT_SEED_GRID_FACTOR(f0_launch, C->seed.f0, R.sf, R.sin)
        }
    }
#define SCAN_TILE_REC
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_REC
    const ConstF64 sfk = (ConstF64) (unsigned long long) H.seed_fk;

    // the lengths under which the checking pass found this ray failing: it stays out of their records
    const unsigned marked = (safe_skip && have) ? mark[ridx] : 0u;
    unsigned code = 0u, marks = 0u; // OR of this ray's codes over the lengths; lengths (bit j - 1) it fails at with -2 / -3

    for (int j0 = 0; j0 < L; j0 += LCH) {
        // (what is live across the frequency loop per length: two cells and one sum; the seed factor is f0_launch or 0, the
        // sign test and `live` are one bit each)
        int pix[LCH], ang[LCH];
        double angsum[LCH];
        unsigned live = 0u, seeded = 0u, neg = 0u; // bit li: the ray is live at / carries its seed factor at / has had a negative Iv at length j0 + li + 1
        bool any_live = false;
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            const int j = j0 + li + 1; // the length, 1-based
            pix[li]     = -1;
            ang[li]     = -1;
            angsum[li]  = 0.0;
            if (j <= L) {
                // the state that serves length j; pixel and angle cell of the exit state
#define SCAN_STATE_SEG j
#define SCAN_STATE_REPORT(b) atomicOr(&H.ctl->len_code[b], 1u << 1);
#define SCAN_STATE_PLACED                                                                                        \
    if (!(fl & F_SKIP) && !((marked >> (j - 1)) & 1u)) {                                                         \
        live |= 1u << li;                                                                                        \
        pix[li] = P.pix;                                                                                         \
        ang[li] = P.ang;                                                                                         \
        if (!(flj & F_ESCAPED)) /* (an escaped ray's seed factor is 0, Helper.h:523-533) */                     \
            seeded |= 1u << li;                                                                                  \
    }
#define SCAN_STATE_FORWARD
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_FORWARD
#undef SCAN_STATE_SEG
#undef SCAN_STATE_REPORT
#undef SCAN_STATE_PLACED
                any_live = any_live || ((live >> li) & 1u);
            }
            // (one placement after the other: interleaved, the four chains of loads of place_ray cost more registers than the
            // frequency loop has to spare)
            asm volatile("" ::: "memory");
        }
        if (__ballot(any_live) == 0ull)
            continue;

        const int s_lo = j0 * RT_N_SUB; // the slots below the chunk: integrated again, nothing deposited
#define SCAN_WALK_SUM(r) angsum[li]
#define SCAN_WALK_DEPOSITS(r) pix[li] >= 0
        if (EMIS) {
#define SCAN_WALK_EMISSION
#include "rt_step_scan_walk.inc"
#undef SCAN_WALK_EMISSION
        } else {
#define SCAN_WALK_SEED
#include "rt_step_scan_walk.inc"
#undef SCAN_WALK_SEED
        }
#undef SCAN_WALK_SUM
#undef SCAN_WALK_DEPOSITS
        // ---- per length of the chunk: the close of its record (rt_step_scan_close.inc) ----
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            if (j0 + li < L) {
                const int jb = j0 + li; // block and bit of this length
                const int px = pix[li];
#define SCAN_CLOSE_SUM angsum[li]
#define SCAN_CLOSE_BIT li
#define SCAN_CLOSE_LIVE ((live >> li) & 1u)
#define SCAN_CLOSE_CODE H.ctl->len_code[jb]
#define SCAN_CLOSE_MARK marks |= 1u << jb;
#define SCAN_CLOSE_TEST
#include "rt_step_scan_close.inc"
#undef SCAN_CLOSE_TEST
#undef SCAN_CLOSE_BIT
#undef SCAN_CLOSE_LIVE
#undef SCAN_CLOSE_CODE
#undef SCAN_CLOSE_MARK
                if (!safe_check) {
#define SCAN_CLOSE_RUNS // the runs of equal pixel AT THIS LENGTH
#define SCAN_CLOSE_OK !failing
#define SCAN_CLOSE_BLOCK jb
#define SCAN_CLOSE_ANG ang[li]
#define SCAN_CLOSE_PIX px
#define SCAN_CLOSE_SCALE H.scale
#define SCAN_CLOSE_DEPOSIT
#include "rt_step_scan_close.inc"
#undef SCAN_CLOSE_DEPOSIT
#undef SCAN_CLOSE_RUNS
#undef SCAN_CLOSE_OK
#undef SCAN_CLOSE_BLOCK
#undef SCAN_CLOSE_ANG
#undef SCAN_CLOSE_PIX
#undef SCAN_CLOSE_SCALE
                }
#undef SCAN_CLOSE_SUM
            }
        }
    }
    if (code) { // one report per ray, whatever the number of lengths it fails at
        report_failure(code);
        if (safe_check && marks)
            mark[ridx] = marks; // the lane that holds the ray writes all its bits
    }
}

template <bool EMIS>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_step_scan_kernel(const ScanKArg A)
{
#define SCAN_WG_KARG ScanKArg
#define SCAN_WG_NREC H.L
#define SCAN_WG_TILES_PER_FETCH (EMIS ? FREQ_TILES_PER_FETCH_EMIS : FREQ_TILES_PER_FETCH_GAIN)
#define SCAN_WG_TILE step_scan_tile<EMIS>
#include "rt_step_scan_wg.inc"
#undef SCAN_WG_KARG
#undef SCAN_WG_NREC
#undef SCAN_WG_TILES_PER_FETCH
#undef SCAN_WG_TILE
}

} // namespace rt
