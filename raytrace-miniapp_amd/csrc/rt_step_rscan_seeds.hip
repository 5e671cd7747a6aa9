#pragma once
// rt_step_rscan_seeds.hip -- step mode of a SEEDED backward plan with a suffix scan AND the seeds of that scan
// (rt_hip_plan_set_suffix_seeds): the step record of every seed beam s < n_seed <= RT_N_SEED_MAX of the run of the LAST n
// lengths, n = 2 .. N, from ONE backward march.
//
// The premises are those of rt_step_scan_seeds.hip and rt_step_rscan.hip: neither the march nor the boundary states depend on
// the seed, which enters as Iv[k] = f0_s f_s[4][k] exp(gl[k]) only, and the backward run of N lengths begins with the run of
// the last n.  The march is the suffix-scan march of the seeded plan unchanged (MODE 0, MARCH_OPT_SCAN);
// rt_step_rscan_seeds_kernel stands where rt_step_rscan_kernel<false> stands and leaves n_seed L records, record
// (s, n) = block s L + (n - 2) -- a seed's curve is contiguous, the layout of rt_step_scan_seeds.hip, whose argument block
// this kernel takes:
//   (s, n)   what rt_step_rscan_kernel<false> leaves for n on a plan of the same problem created with seed s:
//            Iv[k] = f0_{s,n} f_s[4][k] exp(gl_n[k]), multiplied in that kernel's order, gl_n the f64 product sum over the
//            suffix's slots in slot order, the seed factor at the position and exit angles of the state that serves record n
//            (the table of rt_step_rscan.hip; rscan_seed_factor), 0 where the ray has escaped by m = n - 1; the plan's scale
// The creation seed is not among the seeds (rt_step_scan_seeds.hip).  The kernel is made of the fragments of the scan
// passes: the shell (rt_step_scan_wg.inc), the tile preamble with the placement at the LAUNCH ray, once per tile for all
// records (rt_step_scan_tile.inc), per chunk and record the serving state, read where it lies, and one seed factor per seed
// (rt_step_scan_state.inc), the backward walk with a seed set, chunks of RSCAN_SEEDS_LCH start segments
// (rt_step_rscan_walk.inc), and per (seed, record) the close (rt_step_scan_close.inc).  What is held across the
// frequency loop per accumulator is the running gl (8 registers) and per seed a factor and a sum (4 each).  With three start
// segments per walk at two seeds the kernel takes 127 VGPRs, none spilled, no scratch and no stack frame -- four waves per
// SIMD; with two it takes 123, with four it spills five and keeps 32 bytes of scratch.  The marks of the checking repeat are
// read and written chunk by chunk: held across the walks as rt_step_scan_seeds.hip holds them (two 64-bit words) the kernel
// spilled four VGPRs at three segments (profiles/suffix_seeds_kernel_resources.txt has what the compiler made of each).
//
// A ray is live for (s, n) exactly when rt_step_rscan_kernel<false> holds it live for n: it has a record, the serving state
// is not under error -1, it is not marked F_SKIP and the checking repeat has not marked it under (s, n).
//
// Failures follow the reference run once per (seed, n): error -1 of the state that serves n keeps the ray out of every
// (s, n) and sets bit 1 in each of their codes; error -2 / -3 under (s, n) removes the ray from (s, n) only.  A failing ray
// is reported once, with the OR of its codes; DevCtl::seed_len_code[s][n - 2] holds the code of (s, n).  The mark of the
// checking repeat is that of rt_step_scan_seeds.hip: bit 32 s + (n - 2) of a 64-bit word per ray, written by the lane that
// holds the ray.
#include "rt_step_rscan.hip"
#include "rt_step_scan_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int RSCAN_SEEDS_LCH = 3; // suffixes (start segments) per walk over a tile

__device__ __forceinline__ void step_rscan_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, ScanSetPtr Z, const int n_seed,
                                                      double *lds_iang, double *lds_ev, const double *tab, double *xpose, const unsigned tile,
                                                      const int lane)
{
    constexpr int SF  = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH = RSCAN_SEEDS_LCH;
    constexpr int NS  = RT_N_SEED_MAX;
#define SCAN_TILE_BACKWARD true // the backward method: the suffix scan takes no other
#define SCAN_TILE_MARK unsigned long long // one word per ray: bit 32 s + (n - 2)
#define SCAN_TILE_HEAD
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_HEAD
#undef SCAN_TILE_BACKWARD
#undef SCAN_TILE_MARK
    // one placement for all records, as step_rscan_tile takes it (the seed factors are per record, below)
#define SCAN_TILE_PLACED !(fl & F_SKIP)
#define SCAN_TILE_LAUNCH_PLACE
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_LAUNCH_PLACE
#undef SCAN_TILE_PLACED
#define SCAN_TILE_REC
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_REC

    unsigned code = 0u; // OR of this ray's codes over seeds and n
    // (the marks of the checking repeat are read and written chunk by chunk, a chunk's records are its own: two 64-bit words
    // that need not live across the frequency loops, as rt_step_rscan_ase_seeds.hip keeps its four)

    static_assert(NS * LCH <= 16, "live and neg keep one bit per (seed, accumulator)");
    for (int a0 = 0; a0 < L; a0 += LCH) {
        // accumulator i of the chunk: the suffix whose first slot is 3 (a0 + i) -- the run of m = L - (a0 + i) marched
        // segments, record n = m + 1, block (within a seed's curve) and bit m - 1
        double angsum[NS][LCH], f0[NS][LCH];
        unsigned live = 0u, neg = 0u; // bit s * LCH + i: the ray is live under / has had a negative Iv under record (s, .) of accumulator i
#pragma unroll
        for (int i = 0; i < LCH; i++) {
#pragma unroll
            for (int s = 0; s < NS; s++) {
                angsum[s][i] = 0.0;
                f0[s][i]     = 0.0;
            }
            if (a0 + i < L) {
                const int mseg = L - (a0 + i);
                // the state that serves this record (error -1 under n whatever the seed: out of every record (s, n))
#define SCAN_STATE_SEG mseg
#define SCAN_STATE_REPORT(b)                                                                                     \
    _Pragma("unroll") for (int s = 0; s < NS; s++) if (s < n_seed) atomicOr(&H.ctl->seed_len_code[s][b], 1u << 1);
#define SCAN_STATE_READ
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_READ
                if (have && !e1 && !(fl & F_SKIP)) {
                    // the (seed, n) pairs under which the checking pass found this ray failing: it stays out of their records
                    const unsigned long long marked = safe_skip ? mark[ridx] : 0ull;
                    unsigned lv = 0u;
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (s < n_seed && !((marked >> (32 * s + mseg - 1)) & 1ull))
                            lv |= 1u << (s * LCH + i);
                    }
                    live |= lv;
#define SCAN_STATE_FACTORS
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_FACTORS
                }
#undef SCAN_STATE_SEG
#undef SCAN_STATE_REPORT
            }
            // (one state after the other, as rt_step_scan.hip places one length after the other)
            asm volatile("" ::: "memory");
        }
        if (__ballot(live != 0u) == 0ull)
            continue;

#define RSCAN_WALK_REC(s) s
#define RSCAN_WALK_SUM(s) angsum[s][i]
#define RSCAN_WALK_SEEDS
#include "rt_step_rscan_walk.inc"
#undef RSCAN_WALK_SEEDS
#undef RSCAN_WALK_REC
#undef RSCAN_WALK_SUM
        // ---- per (seed, record) of the chunk: its close (rt_step_scan_close.inc) ----
#pragma unroll
        for (int i = 0; i < LCH; i++) {
            if (a0 + i < L) {
                const int jb = L - 1 - (a0 + i); // block (within a seed's curve) and bit of this n
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
                        const bool lv = ((live >> (s * LCH + i)) & 1u) != 0u;
#define SCAN_CLOSE_SUM angsum[s][i]
#define SCAN_CLOSE_BIT s * LCH + i
#define SCAN_CLOSE_LIVE lv
#define SCAN_CLOSE_CODE H.ctl->seed_len_code[s][jb]
                        // (the lane that holds the ray writes its bits, chunk by chunk)
#define SCAN_CLOSE_MARK                                                                                          \
    if (safe_check)                                                                                              \
        mark[ridx] |= 1ull << (32 * s + jb);
#define SCAN_CLOSE_TEST
#include "rt_step_scan_close.inc"
#undef SCAN_CLOSE_TEST
#undef SCAN_CLOSE_BIT
#undef SCAN_CLOSE_LIVE
#undef SCAN_CLOSE_CODE
#undef SCAN_CLOSE_MARK
                        if (!safe_check) {
#define SCAN_CLOSE_OK lv && !failing
#define SCAN_CLOSE_BLOCK s * L + jb
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
        }
    }
    if (code) // one report per ray, whatever the number of seeds and n it fails under
        report_failure(code);
}

// (the launch bounds of rt_step_rscan_kernel<false>)
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_step_rscan_seeds_kernel(const ScanSeedsKArg A)
{
#define SCAN_WG_KARG ScanSeedsKArg
#define SCAN_WG_NREC A.set.n_seed * H.L
#define SCAN_WG_TILES_PER_FETCH FREQ_TILES_PER_FETCH_GAIN
#define SCAN_WG_SET ScanSetPtr
#define SCAN_WG_TILE step_rscan_seeds_tile
#include "rt_step_scan_wg.inc"
#undef SCAN_WG_KARG
#undef SCAN_WG_NREC
#undef SCAN_WG_TILES_PER_FETCH
#undef SCAN_WG_SET
#undef SCAN_WG_TILE
}

} // namespace rt
