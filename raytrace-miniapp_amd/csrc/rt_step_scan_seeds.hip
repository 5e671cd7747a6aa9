#pragma once
// rt_step_scan_seeds.hip -- step mode with a length scan AND the seeds of the scan (rt_hip_plan_set_scan_seeds): the step
// record of every seed beam s < n_seed <= RT_N_SEED_MAX at every plasma length n = 2 .. N from ONE forward march.
//
// Neither the march nor the boundary states depend on the seed (rt_step_seeds.hip, rt_step_scan.hip say why): the seed enters
// as Iv[k] = f0_s f_s[4][k] exp(gl[k]) only, and exp(gl_j[k]) of length j is the same for every seed.  rt_step_scan_seeds_kernel
// stands where rt_step_scan_kernel stands, gain-only (an emission plan has no seed), and is made of the same fragments: the
// shell (rt_step_scan_wg.inc) with n_rec = n_seed L records, record (s, j) = block s L + (j - 1) -- a seed's curve is
// contiguous --, the tile preamble and the per-seed factor at the launch ray (rt_step_scan_tile.inc), the state that serves
// length j (rt_step_scan_state.inc), the forward walk with a seed set (rt_step_scan_walk.inc: exp_tab_vec ONCE per length,
// then Iv per seed, so every Iv_{s,j}[k] is the double a plain scan plan created with seed s computes) and the close of a
// record (rt_step_scan_close.inc).  At the end of a chunk, per length: the failure tests of all seeds, the runs of equal pixel
// once (rt_wave_runs.inc), then per seed the I_ang add and the segmented nf scan.
//
// The lengths are taken in chunks of SCAN_SEEDS_LCH = 2 (rt_step_scan_kernel: 4): what is live per (seed, length) across the
// frequency loop is the sum over k, a double; RT_N_SEED_MAX x 2 of them are the four the plain scan kernel holds, with the
// second seed's launch factor in place of two of its four pixel / angle cells.  A chunk re-integrates the slots below it --
// 6 (c - 1) for chunk c, a product sum per slot in this mode, no exponential.  Seed and length loops are unrolled under
// wave-uniform tests: nothing per (seed, length) is indexed memory.
//
// Failures follow the reference run once per seed and length: error -1 depends on neither -- s.z^2 < 0.01 of the state that
// serves length j sets bit 1 in the code of (s, j) for every s; error -2 / -3 under seed s at length j removes the ray from
// record (s, j) only.  A ray that fails anywhere is reported once, with the OR of its codes;
// DevCtl::seed_len_code[s][j - 1] holds the code of (s, j).  The checking repeat keeps its two passes; the mark of a ray is
// one bit per (seed, length), bit 32 s + (j - 1) of a 64-bit word per ray (FreqHot::bad is an array of such words here),
// written by the one lane that holds the ray.
#include "rt_step_scan.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int SCAN_SEEDS_LCH = 2; // lengths per pass over a tile
static_assert(RT_N_SEED_MAX * 32 <= 64 && RT_N_SCAN_MAX <= 32, "one mark bit per (seed, length) in a 64-bit word per ray");

// the seeds of a scan: what rt_step_scan_seeds_kernel reads beside the blocks of rt_step_scan_kernel (through the constant
// address space, where it is needed)
struct ScanSeedsArg {
    int n_seed;
    int pad;
    SeedTabs tabs;
};
static_assert(offsetof(ScanSeedsArg, tabs) == 8 && sizeof(ScanSeedsArg) == 8 + sizeof(SeedTabs), "nesting SeedTabs moves no byte of the argument block");
struct ScanSeedsKArg {
    FreqHot hot;
    FreqCold cold;
    ScanArg scan; // out: n_seed L blocks, block s L + (j - 1) the record of seed s at length j
    ScanSeedsArg set;
};
typedef const RT_CONST_AS ScanSeedsArg *ScanSetPtr;

__device__ __forceinline__ void step_scan_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, ScanSetPtr Z, const int n_seed,
                                                     double *lds_iang, double *lds_ev, const double *tab, double *xpose, const unsigned tile,
                                                     const int lane)
{
    constexpr int SF  = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH = SCAN_SEEDS_LCH;
    constexpr int NS  = RT_N_SEED_MAX;
#define SCAN_TILE_BACKWARD false // the forward method: the scan takes no other
#define SCAN_TILE_MARK unsigned long long
#define SCAN_TILE_HEAD
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_HEAD
#undef SCAN_TILE_BACKWARD
#undef SCAN_TILE_MARK
#define SCAN_TILE_ON_GRID R.sf
#define SCAN_TILE_LAUNCH_FACTORS
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_LAUNCH_FACTORS
#undef SCAN_TILE_ON_GRID
#define SCAN_TILE_REC
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_REC

    // the (seed, length) pairs under which the checking pass found this ray failing: it stays out of their records
    const unsigned long long marked = (safe_skip && have) ? mark[ridx] : 0ull;
    unsigned code            = 0u;   // OR of this ray's codes over seeds and lengths
    unsigned long long marks = 0ull; // (seed, length) pairs (bit 32 s + j - 1) it fails at with -2 / -3

    for (int j0 = 0; j0 < L; j0 += LCH) {
        int pix[LCH], ang[LCH];
        double angsum[NS][LCH];
        // bit li: the ray is live at / carries its seed factors at length j0 + li + 1; bit s LCH + li: a negative Iv seen under
        // seed s at that length / the ray is marked under (s, that length)
        unsigned live = 0u, seeded = 0u, neg = 0u, out = 0u;
        bool any_live = false;
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            const int j = j0 + li + 1; // the length, 1-based
            pix[li]     = -1;
            ang[li]     = -1;
#pragma unroll
            for (int s = 0; s < NS; s++)
                angsum[s][li] = 0.0;
            if (j <= L) {
                // the state that serves length j (error -1 whatever the seed: out of every record (s, j)); pixel and angle
                // cell of the exit state
#define SCAN_STATE_SEG j
#define SCAN_STATE_REPORT(b)                                                                                     \
    _Pragma("unroll") for (int s = 0; s < NS; s++) if (s < n_seed) atomicOr(&H.ctl->seed_len_code[s][b], 1u << 1);
#define SCAN_STATE_PLACED                                                                                        \
    if (!(fl & F_SKIP)) {                                                                                        \
        live |= 1u << li;                                                                                        \
        pix[li] = P.pix;                                                                                         \
        ang[li] = P.ang;                                                                                         \
        if (!(flj & F_ESCAPED)) /* (an escaped ray's seed factor is 0, Helper.h:523-533) */                     \
            seeded |= 1u << li;                                                                                  \
        _Pragma("unroll") for (int s = 0; s < NS; s++)                                                           \
            out |= ((marked >> (32 * s + j - 1)) & 1ull) ? 1u << (s * LCH + li) : 0u;                            \
    }
#define SCAN_STATE_FORWARD
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_FORWARD
#undef SCAN_STATE_SEG
#undef SCAN_STATE_REPORT
#undef SCAN_STATE_PLACED
                any_live = any_live || ((live >> li) & 1u);
            }
            // (one placement after the other, as in rt_step_scan.hip)
            asm volatile("" ::: "memory");
        }
        if (__ballot(any_live) == 0ull)
            continue;

        const int s_lo = j0 * RT_N_SUB; // the slots below the chunk: integrated again, nothing deposited
#define SCAN_WALK_REC(s) s
#define SCAN_WALK_SUM(r) angsum[r][li]
#define SCAN_WALK_DEPOSITS(r) pix[li] >= 0 && !((out >> (r * LCH + li)) & 1u)
#define SCAN_WALK_SEEDS
#include "rt_step_scan_walk.inc"
#undef SCAN_WALK_SEEDS
#undef SCAN_WALK_REC
#undef SCAN_WALK_SUM
#undef SCAN_WALK_DEPOSITS
        // ---- per length of the chunk: per seed the failure test; the runs of equal pixel once; per seed the deposit
        // (rt_step_scan_close.inc) ----
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            if (j0 + li < L) {
                const int jb  = j0 + li; // block (within a seed's curve) and bit of this length
                const int px  = pix[li];
                const bool dp = px >= 0;
                unsigned failing_s = 0u; // bit s: the ray fails under seed s at this length
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
#define SCAN_CLOSE_SUM angsum[s][li]
#define SCAN_CLOSE_BIT s * LCH + li
#define SCAN_CLOSE_LIVE ((live >> li) & 1u)
#define SCAN_CLOSE_CODE H.ctl->seed_len_code[s][jb]
#define SCAN_CLOSE_MARK marks |= 1ull << (32 * s + jb);
#define SCAN_CLOSE_FAILS failing_s |= 1u << s;
#define SCAN_CLOSE_TEST
#include "rt_step_scan_close.inc"
#undef SCAN_CLOSE_TEST
#undef SCAN_CLOSE_BIT
#undef SCAN_CLOSE_LIVE
#undef SCAN_CLOSE_CODE
#undef SCAN_CLOSE_MARK
#undef SCAN_CLOSE_FAILS
                    }
                }
                if (!safe_check) {
#define RUNS_PIX px
#define RUNS_DEPOSITS dp
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (s < n_seed) {
                            const bool ok = !((failing_s >> s) & 1u) && !((out >> (s * LCH + li)) & 1u);
#define SCAN_CLOSE_OK ok
#define SCAN_CLOSE_BLOCK s * L + jb
#define SCAN_CLOSE_ANG ang[li]
#define SCAN_CLOSE_PIX px
#define SCAN_CLOSE_SCALE H.scale
#define SCAN_CLOSE_DEPOSIT
#include "rt_step_scan_close.inc"
#undef SCAN_CLOSE_DEPOSIT
#undef SCAN_CLOSE_OK
#undef SCAN_CLOSE_BLOCK
#undef SCAN_CLOSE_ANG
#undef SCAN_CLOSE_PIX
#undef SCAN_CLOSE_SCALE
#undef SCAN_CLOSE_SUM
                        }
                    }
                }
            }
        }
    }
    if (code) { // one report per ray, whatever the number of seeds and lengths it fails at
        report_failure(code);
        if (safe_check && marks)
            mark[ridx] = marks; // the lane that holds the ray writes all its bits
    }
}

__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_step_scan_seeds_kernel(const ScanSeedsKArg A)
{
#define SCAN_WG_KARG ScanSeedsKArg
#define SCAN_WG_NREC A.set.n_seed * H.L
#define SCAN_WG_TILES_PER_FETCH FREQ_TILES_PER_FETCH_GAIN
#define SCAN_WG_SET ScanSetPtr
#define SCAN_WG_TILE step_scan_seeds_tile
#include "rt_step_scan_wg.inc"
#undef SCAN_WG_KARG
#undef SCAN_WG_NREC
#undef SCAN_WG_TILES_PER_FETCH
#undef SCAN_WG_SET
#undef SCAN_WG_TILE
}

} // namespace rt
