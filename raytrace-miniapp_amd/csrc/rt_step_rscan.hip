#pragma once
// rt_step_rscan.hip -- step mode with a suffix scan (rt_hip_plan_enable_suffix_scan): the step record of the run of the LAST
// n lengths, n = 2 .. N, from ONE backward march.
//
// With the backward method RayTrace_calc_ray starts at the launch ray and walks the lengths ii = N - 1, N - 2, ..., 1
// (Helper.h:430-441): its first n - 1 outer iterations are the whole run of the problem that holds gain[0] and the last
// n - 1 lengths (problem.suffix_lengths), so slots 3 (N - n) .. 3 (N - 1) - 1 of the march record of the N-run are the
// whole record of that run, and the state it ends with is the state with which the ray left its m = n - 1 first marched
// segments: boundary m of the scan instance of the march (rt_march.hip, MARCH_OPT_SCAN: the store is indexed by the number
// of segments marched, whatever the method).  Which state serves record n, with m = n - 1, and error -1 under it:
// rt_step_scan_state.inc.  The seed factor (gain-only mode) is taken at that state's position and exit angles
// (Helper.h:525-529) and is 0 where the ray has escaped by m.  The backward method deposits at the LAUNCH ray
// (RayTraceImageCPU.cpp:37-39): pixel, angle cell and the runs of equal pixel of a tile are the same for every record and
// are taken once (rt_step_scan_tile.inc).
//
// rt_step_rscan_kernel stands where rt_step_scan_kernel stands and has its shell (rt_step_scan_wg.inc), its tile preamble
// (rt_step_scan_tile.inc) and its close of a record (rt_step_scan_close.inc).  What differs is the walk
// (rt_step_rscan_walk.inc): the suffixes are taken in chunks of LCH start segments, ONE walk per frequency batch with LCH
// accumulators that join one after the other; chunk c = 0, 1, ... walks 3 LCH c slots fewer than the first.  ase_factor
// and ase_update_call below are what that walk takes in place of ase_step and ase_update.
//
// The chunk: the launch bounds allow 128 VGPRs (four waves per SIMD).  An accumulator is 8 of them, the sum over k of a
// record 2, its seed factor (gain-only) 2; pixel, angle cell and run structure are held once.  Emission takes
// RSCAN_LCH_EMIS = 4 (118 VGPRs, no scratch), gain-only RSCAN_LCH_GAIN = 3 (117 VGPRs, no scratch; with four the instance
// is at 126 and keeps a 48-byte frame, as rt_step_scan_kernel once did with a fourth inlined seed factor).
// profiles/suffix_scan_kernel_resources.txt has what the compiler made of both.
//
// Failures follow the reference run once per record, as in rt_step_scan.hip: error -1 under record n sets bit 1 of that
// record's code and keeps the ray out of record n; error -2 / -3 under record n removes the ray from record n only.  A ray
// that fails anywhere is reported once, with the OR of its codes; DevCtl::len_code[n - 2] holds the code of record n.  The
// mark of the checking repeat is one bit per record in a 32-bit word.  The probe's exit ray, flags and steps are those of
// the whole run.
#include "rt_step_scan.hip"

#include <type_traits>

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int RSCAN_LCH_EMIS = 4, RSCAN_LCH_GAIN = 3; // suffixes (start segments) per walk over a tile

// e^gl - 1 of a regular sub-segment for VEC frequencies: ase_step (rt_freq.hip) up to its last line, statement by
// statement; apply(j, em1) stands where ase_step has Iv[j] = fma(em1, Iv[j] + rs, Iv[j]) and does that for every accumulator
// that takes the factor, so each of them is ase_step's Iv.  (The factor is handed over frequency by frequency, as ase_step
// consumes it: four of them held beside the accumulators are six more registers alive across the updates.)
template <typename Apply> __device__ __forceinline__ void ase_factor(const float gs, const float (&w)[VEC], const double *tab, Apply apply)
{
    const double L2E   = 369.3299304675746;     // 256 / ln 2
    const double LN2_N = 0.0027076061740622863; // ln 2 / 256
    const double MAGIC = 0x1.8p52;              // adding it leaves rint(.) in the low mantissa bits
    double rq[VEC], T[VEC];
    int m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        const double x = (double) (gs * w[j]);
        double t       = fma(x, L2E, MAGIC);
        const int n    = __double2loint(t);
        t -= MAGIC;
        rq[j] = fma(-t, LN2_N, x);
        T[j]  = tab[n & (EXP_TAB - 1)];
        m[j]  = n >> 8;
    }
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        double q = fma(rq[j], 1.0 / 6.0, 0.5);
        q        = fma(rq[j], q, 1.0);
        rq[j] *= q;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        int hi; // exponent field += m (ase_step's instruction)
        asm("v_lshl_add_u32 %0, %1, 20, %2" : "=v"(hi) : "v"(m[j]), "v"(__double2hiint(T[j])));
        const double S = __hiloint2double(hi, __double2loint(T[j]));
        apply(j, fma(S, rq[j], S - 1.0));
    }
}

// ase_update (rt_freq.hip) held to a call, as scan_seed_factor holds pchip_eval: the update of the irregular sub-segments
// and of the exact mode, the same statements and hence the same double
static __device__ __attribute__((noinline)) double ase_update_call(double Iv, float gs, float es, float w, const double *tab)
{
    return ase_update(Iv, gs, es, w, tab);
}

// scan_seed_factor (rt_step_scan.hip), statement by statement, on a seed that stays in the argument block: every table
// pointer and dimension is read through the constant address space where it is used, not as a copy of the whole DevSeed
// held in scalar registers across the four calls (with the copy the kernel kept a stack frame that nothing read).  The
// kernels that carry the seeds of a suffix scan take it (rt_step_rscan_ase_seeds.hip, rt_step_rscan_seeds.hip).
__device__ __forceinline__ double rscan_seed_factor(const RT_CONST_AS DevSeed *sd, double x, double y, double a, double b)
{
    auto xs  = [&](int d) { return (ConstF64) (unsigned long long) sd->x[d]; };
    auto fs  = [&](int d) { return reinterpret_cast<const double *>((unsigned long long) sd->f[d]); };
    double f = 0.0;
    if (x >= xs(0)[0] && x <= xs(0)[sd->dim[0] - 1] && y >= xs(1)[0] && y <= xs(1)[sd->dim[1] - 1] && a >= xs(2)[0] &&
        a <= xs(2)[sd->dim[2] - 1] && b >= xs(3)[0] && b <= xs(3)[sd->dim[3] - 1]) {
        double fx, fy, fa, fb;
        [[clang::noinline]] fx = pchip_eval(sd->dim[0], reinterpret_cast<const double *>((unsigned long long) sd->x[0]), fs(0), x);
        [[clang::noinline]] fy = pchip_eval(sd->dim[1], reinterpret_cast<const double *>((unsigned long long) sd->x[1]), fs(1), y);
        [[clang::noinline]] fa = pchip_eval(sd->dim[2], reinterpret_cast<const double *>((unsigned long long) sd->x[2]), fs(2), a);
        [[clang::noinline]] fb = pchip_eval(sd->dim[3], reinterpret_cast<const double *>((unsigned long long) sd->x[3]), fs(3), b);
        f = sd->f0 * fx * fy * fa * fb;
        f = f < 0.0 ? 0.0 : f;
    }
    return f;
}

template <bool EMIS>
__device__ __forceinline__ void step_rscan_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, double *lds_iang, double *lds_ev,
                                                const double *tab, double *xpose, const unsigned tile, const int lane)
{
    constexpr int SF  = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH = EMIS ? RSCAN_LCH_EMIS : RSCAN_LCH_GAIN;
#define SCAN_TILE_BACKWARD true // the backward method: rt_hip_plan_enable_suffix_scan takes no other
#define SCAN_TILE_MARK unsigned
#define SCAN_TILE_HEAD
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_HEAD
#undef SCAN_TILE_BACKWARD
#undef SCAN_TILE_MARK
    // one placement for all records (the seed factor is per record, below)
#define SCAN_TILE_PLACED !(fl & F_SKIP)
#define SCAN_TILE_LAUNCH_PLACE
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_LAUNCH_PLACE
#undef SCAN_TILE_PLACED
#define SCAN_TILE_REC
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_REC
    const ConstF64 sfk = (ConstF64) (unsigned long long) H.seed_fk;

    // the records under which the checking pass found this ray failing: it stays out of them
    const unsigned marked = (safe_skip && have) ? mark[ridx] : 0u;
    unsigned code = 0u, marks = 0u; // OR of this ray's codes over the records; records (bit n - 2) it fails under with -2 / -3

    for (int a0 = 0; a0 < L; a0 += LCH) {
        // accumulator i of the chunk: the suffix whose first slot is 3 (a0 + i) -- the run of m = L - (a0 + i) marched
        // segments, record n = m + 1, block and bit m - 1
        double angsum[LCH], f0[LCH];
        unsigned live = 0u, neg = 0u; // bit i: the ray is live under / has had a negative Iv under the record of accumulator i
        // (the final state again, from memory: five registers that need not live across the frequency loops)
        RecMeta mc = { 0, 0, 0, 0, 1, 0 };
        if (have)
            mc = *reinterpret_cast<const RecMeta *>(rec + rec_meta_off(rrec, S, H.rec_stride));
#pragma unroll
        for (int i = 0; i < LCH; i++) {
            angsum[i] = 0.0;
            f0[i]     = 0.0;
            if (a0 + i < L) {
                const int mseg = L - (a0 + i);
                // the state that serves this record
#define SCAN_STATE_SEG mseg
#define SCAN_STATE_REPORT(b) atomicOr(&H.ctl->len_code[b], 1u << 1);
#define SCAN_STATE_HELD
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_HELD
#undef SCAN_STATE_SEG
#undef SCAN_STATE_REPORT
                if (have && !e1 && !(fl & F_SKIP) && !((marked >> (mseg - 1)) & 1u)) {
                    live |= 1u << i;
                    // the seed factor at this state's position and exit angles (place_ray's backward half, Helper.h:518-529);
                    // 0 where the ray has escaped by m
                    if (!EMIS && (hflags & FQ_HAS_SEED) && !esc) {
                        const float ea   = atanf_flt32_kernel(ssx / ssz) * 1e3f;
                        const float eb   = atanf_flt32_kernel(ssy / ssz) * 1e3f;
                        const DevSeed SD = load_cold(&C->seed);
                        f0[i]            = scan_seed_factor(SD, (double) spx, (double) spy, (double) ea, (double) eb);
                    }
                }
            }
            // (one state after the other, as rt_step_scan.hip places one length after the other)
            asm volatile("" ::: "memory");
        }
        if (__ballot(live != 0u) == 0ull)
            continue;

#define RSCAN_WALK_SUM(s) angsum[i]
        if (EMIS) {
#define RSCAN_WALK_EMISSION
#include "rt_step_rscan_walk.inc"
#undef RSCAN_WALK_EMISSION
        } else {
#define RSCAN_WALK_SEED
#include "rt_step_rscan_walk.inc"
#undef RSCAN_WALK_SEED
        }
#undef RSCAN_WALK_SUM
        // ---- per record of the chunk: its close (rt_step_scan_close.inc) ----
#pragma unroll
        for (int i = 0; i < LCH; i++) {
            if (a0 + i < L) {
                const int jb  = L - 1 - (a0 + i); // block and bit of this record
                const bool lv = ((live >> i) & 1u) != 0u;
#define SCAN_CLOSE_SUM angsum[i]
#define SCAN_CLOSE_BIT i
#define SCAN_CLOSE_LIVE lv
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
#define SCAN_CLOSE_OK lv && !failing
#define SCAN_CLOSE_BLOCK jb
#define SCAN_CLOSE_ANG ang
#define SCAN_CLOSE_PIX pix
#define SCAN_CLOSE_HAS_PIX has_pix
#define SCAN_CLOSE_SCALE H.scale
#define SCAN_CLOSE_DEPOSIT
#include "rt_step_scan_close.inc"
#undef SCAN_CLOSE_DEPOSIT
#undef SCAN_CLOSE_OK
#undef SCAN_CLOSE_BLOCK
#undef SCAN_CLOSE_ANG
#undef SCAN_CLOSE_PIX
#undef SCAN_CLOSE_HAS_PIX
#undef SCAN_CLOSE_SCALE
                }
#undef SCAN_CLOSE_SUM
            }
        }
    }
    if (code) { // one report per ray, whatever the number of records it fails under
        report_failure(code);
        if (safe_check && marks)
            mark[ridx] = marks; // the lane that holds the ray writes all its bits
    }
}

template <bool EMIS>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_step_rscan_kernel(const ScanKArg A)
{
#define SCAN_WG_KARG ScanKArg
#define SCAN_WG_NREC H.L
#define SCAN_WG_TILES_PER_FETCH (EMIS ? FREQ_TILES_PER_FETCH_EMIS : FREQ_TILES_PER_FETCH_GAIN)
#define SCAN_WG_TILE step_rscan_tile<EMIS>
#include "rt_step_scan_wg.inc"
#undef SCAN_WG_KARG
#undef SCAN_WG_NREC
#undef SCAN_WG_TILES_PER_FETCH
#undef SCAN_WG_TILE
}

} // namespace rt
