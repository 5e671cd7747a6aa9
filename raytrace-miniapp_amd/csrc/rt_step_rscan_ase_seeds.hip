#pragma once
// rt_step_rscan_ase_seeds.hip -- step mode of an EMISSION plan with a suffix scan AND ASE seeds of that scan
// (rt_hip_plan_set_suffix_ase_seeds): the whole per-step record -- the ASE triple and one seeded triple per seed beam -- of
// the run of the LAST n lengths, n = 2 .. N, from ONE backward march.
//
// The two premises are those of rt_step_ase_seeds.hip and rt_step_rscan.hip: the march does not depend on the emission
// switch apart from evl and not on the seed at all, and the backward run of N lengths begins with the run of the last n.
// The march is the suffix-scan march unchanged (MODE 1, MARCH_OPT_SCAN); rt_step_rscan_ase_seeds_kernel stands where
// rt_step_rscan_kernel<true> stands and leaves (1 + n_seed) L records, record (r, n) = block r L + (n - 2) -- a record's curve
// is contiguous, the ASE curve first (the layout of rt_step_scan_ase_seeds.hip, whose argument block this kernel takes):
//   (0, n)       what rt_step_rscan_kernel<true> leaves for n on this plan: the shared-factor emission walk (ase_factor,
//                ase_update_call, wnan from the suffix's own first slot on), exact emission honoured, the plan's scale
//   (1 + s, n)   what rt_step_rscan_kernel<false> leaves for n on a plan of the same problem created with seed s: gain-only,
//                Iv[k] = f0_{s,n} f_s[4][k] exp(gl_n[k]), gl_n the f64 product sum over the suffix's slots in slot order, the
//                seed factor at the position and exit angles of the state that serves record n (the table of
//                rt_step_rscan.hip, scan_seed_factor), 0 where the ray has escaped by m = n - 1; scale scales[s]
// The kernel is made of the fragments of the scan passes: the shell (rt_step_scan_wg.inc), the tile preamble with the
// placement at the LAUNCH ray, once per tile for all records (rt_step_scan_tile.inc), the serving state and the seed factors
// (rt_step_scan_state.inc), the backward walk in its emission form and in its form with a seed set (rt_step_rscan_walk.inc)
// and the close of a record (rt_step_scan_close.inc).
//
// Per tile the frequencies are walked in two halves (the HALVES of rt_step_ase_seeds.hip and rt_step_scan_ase_seeds.hip):
//   the emission half   the chunked suffix walk of step_rscan_tile<true>, RSCAN_ASE_LCH_EMIS start segments per walk, and
//                       behind each chunk the failure test, the I_ang add and the nf scan of its records (0, n)
//   the seed half       the gain-only walk, RSCAN_ASE_LCH_SEED start segments per walk: per accumulator the running gl,
//                       n_seed factors and n_seed sums; one gl walk and one ballot-skipped exp_tab_vec per record serve all
//                       seeds; behind each chunk the same three steps per (1 + s, n)
// Nothing of one half is live across the other: the serving state and the seed factors are taken where the seed half
// begins a chunk, the sums of record 0 are spent before it starts.  The emission half is step_rscan_tile<true>'s text and
// keeps its budget with four accumulators (alone it compiles to 116 VGPRs).  The seed half holds per accumulator the
// running gl (8 registers) and per seed a factor and a sum (4 each): with three accumulators the kernel takes 128 VGPRs,
// none spilled, no scratch, no stack frame -- four waves per SIMD; with four it spills six and keeps a 32-byte frame, with
// two it takes 125.  What decided it was not the accumulators but the seed factor: scan_seed_factor on a copy of the
// seed's table block (load_cold) left a 32 .. 48-byte frame at every chunk size, inlined per (seed, accumulator) or in a
// loop over the seeds, and behind a call it spilled; rscan_seed_factor reads the block where it lies
// (profiles/suffix_ase_seeds_kernel_resources.txt has what the compiler made of each).
//
// F_SKIP (rt_step_ase_seeds.hip): a ray whose sums over the whole N-run are all zero is masked from the ASE records only
// and is live for the seed records; a tile none of whose rays is live for record 0 skips the emission half.
//
// Failures follow the reference run once per (record, n): error -1 of the state that serves n keeps the ray out of every
// (r, n) and sets bit 1 in each of their codes (the seed half does that for all records: it runs for every tile); error
// -2 / -3 under (r, n) removes the ray from (r, n) only.  A failing ray is reported once, with the OR of its codes;
// DevCtl::rec_len_code[r][n - 2] holds the code of (r, n).  The mark of the checking repeat is that of
// rt_step_scan_ase_seeds.hip: bit n - 2 of word r of four 32-bit words per ray, written by the lane that holds the ray.
#include "rt_step_rscan.hip"
#include "rt_step_scan_ase_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int RSCAN_ASE_LCH_EMIS = 4, RSCAN_ASE_LCH_SEED = 3; // suffixes (start segments) per walk over a tile, per half

__device__ __forceinline__ void step_rscan_ase_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, ScanAsePtr Z, const int n_seed,
                                                          double *lds_iang, double *lds_ev, const double *tab, double *xpose, const unsigned tile,
                                                          const int lane)
{
    constexpr int SF = 0; // (the text fragments below read it: slots at run time)
    constexpr int NS = RT_N_SEED_MAX;
#define SCAN_TILE_BACKWARD true // the backward method: the suffix scan takes no other
#define SCAN_TILE_MARK unsigned // four words per ray: word r the records (r, n) of the ray, bit n - 2
#define SCAN_TILE_HEAD
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_HEAD
#undef SCAN_TILE_BACKWARD
#undef SCAN_TILE_MARK
    // one placement for all records, as step_rscan_tile takes it -- of a ray marked F_SKIP as well: the seed records take it
#define SCAN_TILE_PLACED true
#define SCAN_TILE_LAUNCH_PLACE
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_LAUNCH_PLACE
#undef SCAN_TILE_PLACED
#define SCAN_TILE_REC
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_REC

    unsigned code = 0u; // OR of this ray's codes over records and n
    // (both halves read the final state again per chunk, from memory: five registers that need not live across the
    // frequency loops, rt_step_rscan.hip)

    // ================= the emission half: records (0, n), the walk of step_rscan_tile<true> =================
    // (a ray marked F_SKIP is not live for record 0: a tile of such rays, or of rays that are out for other reasons, skips it)
    if (__ballot(have && !(fl & F_SKIP)) != 0ull) {
        constexpr int LCH     = RSCAN_ASE_LCH_EMIS;
        const unsigned marked = (safe_skip && have) ? mark[4u * ridx] : 0u;
        for (int a0 = 0; a0 < L; a0 += LCH) {
            // accumulator i of the chunk: the suffix whose first slot is 3 (a0 + i) -- the run of m = L - (a0 + i) marched
            // segments, record n = m + 1, block and bit m - 1
            double angsum[LCH];
            unsigned live = 0u, neg = 0u; // bit i: the ray is live under / has had a negative Iv under the record of accumulator i
            RecMeta mc = { 0, 0, 0, 0, 1, 0 };
            if (have)
                mc = *reinterpret_cast<const RecMeta *>(rec + rec_meta_off(rrec, S, H.rec_stride));
#pragma unroll
            for (int i = 0; i < LCH; i++) {
                angsum[i] = 0.0;
                if (a0 + i < L) {
                    const int mseg = L - (a0 + i);
                    // the state that serves this record: sz is all this half reads of it (error -1 is reported by the seed half,
                    // for every record)
#define SCAN_STATE_SEG mseg
#define SCAN_STATE_SILENT
#define SCAN_STATE_HELD
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_HELD
#undef SCAN_STATE_SILENT
#undef SCAN_STATE_SEG
                    if (have && !e1 && !(fl & F_SKIP) && !((marked >> (mseg - 1)) & 1u))
                        live |= 1u << i;
                }
                asm volatile("" ::: "memory");
            }
            if (__ballot(live != 0u) == 0ull)
                continue;

#define RSCAN_WALK_SUM(s) angsum[i]
#define RSCAN_WALK_EMISSION
#include "rt_step_rscan_walk.inc"
#undef RSCAN_WALK_EMISSION
#undef RSCAN_WALK_SUM
            // ---- per record of the chunk: its close (rt_step_scan_close.inc) ----
#pragma unroll
            for (int i = 0; i < LCH; i++) {
                if (a0 + i < L) {
                    const int jb  = L - 1 - (a0 + i); // block (within the ASE curve) and bit of this record
                    const bool lv = ((live >> i) & 1u) != 0u;
#define SCAN_CLOSE_SUM angsum[i]
#define SCAN_CLOSE_BIT i
#define SCAN_CLOSE_LIVE lv
#define SCAN_CLOSE_CODE H.ctl->rec_len_code[0][jb]
                    // (the lane that holds the ray writes its bits, chunk by chunk: a chunk's records are its own)
#define SCAN_CLOSE_MARK                                                                                          \
    if (safe_check)                                                                                              \
        mark[4u * ridx] |= 1u << jb;
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
    }

    // ================= the seed half: records (1 + s, n), the walk of step_rscan_seeds_tile, each record with its scale =================
    {
        constexpr int LCH = RSCAN_ASE_LCH_SEED;
        static_assert(NS * LCH <= 16, "live and neg keep one bit per (seed, accumulator)");
        for (int a0 = 0; a0 < L; a0 += LCH) {
            double angsum[NS][LCH], f0[NS][LCH];
            unsigned live = 0u, neg = 0u; // bit s * LCH + i: the ray is live under / has had a negative Iv under record (1 + s, .) of accumulator i
#pragma unroll
            for (int i = 0; i < LCH; i++) {
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    angsum[s][i] = 0.0;
                    f0[s][i]     = 0.0;
                }
                if (a0 + i < L) {
                    const int mseg = L - (a0 + i);
                    // the state that serves this record (error -1 under n whatever the record: out of every record (r, n))
#define SCAN_STATE_SEG mseg
#define SCAN_STATE_REPORT(b)                                                                                     \
    _Pragma("unroll") for (int r = 0; r < 1 + NS; r++) if (r <= n_seed) atomicOr(&H.ctl->rec_len_code[r][b], 1u << 1);
#define SCAN_STATE_READ
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_READ
                    if (have && !e1) {
                        unsigned lv = 0u;
#pragma unroll
                        for (int s = 0; s < NS; s++) {
                            if (s < n_seed) {
                                const unsigned marked = safe_skip ? mark[4u * ridx + 1u + (unsigned) s] : 0u;
                                if (!((marked >> (mseg - 1)) & 1u))
                                    lv |= 1u << (s * LCH + i);
                            }
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

#define RSCAN_WALK_REC(s) (1 + s)
#define RSCAN_WALK_SUM(s) angsum[s][i]
#define RSCAN_WALK_SCALE(s) Z->scale[1 + s]
#define RSCAN_WALK_SEEDS
#include "rt_step_rscan_walk.inc"
#undef RSCAN_WALK_SEEDS
#undef RSCAN_WALK_REC
#undef RSCAN_WALK_SUM
#undef RSCAN_WALK_SCALE
            // ---- per (seed, record) of the chunk: its close (rt_step_scan_close.inc) ----
#pragma unroll
            for (int i = 0; i < LCH; i++) {
                if (a0 + i < L) {
                    const int jb = L - 1 - (a0 + i); // block (within a record's curve) and bit of this n
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (s < n_seed) {
                            const bool lv = ((live >> (s * LCH + i)) & 1u) != 0u;
#define SCAN_CLOSE_SUM angsum[s][i]
#define SCAN_CLOSE_BIT s * LCH + i
#define SCAN_CLOSE_LIVE lv
#define SCAN_CLOSE_CODE H.ctl->rec_len_code[1 + s][jb]
#define SCAN_CLOSE_MARK                                                                                          \
    if (safe_check)                                                                                              \
        mark[4u * ridx + 1u + (unsigned) s] |= 1u << jb;
#define SCAN_CLOSE_TEST
#include "rt_step_scan_close.inc"
#undef SCAN_CLOSE_TEST
#undef SCAN_CLOSE_BIT
#undef SCAN_CLOSE_LIVE
#undef SCAN_CLOSE_CODE
#undef SCAN_CLOSE_MARK
                            if (!safe_check) {
#define SCAN_CLOSE_OK lv && !failing
#define SCAN_CLOSE_BLOCK (1 + s) * L + jb
#define SCAN_CLOSE_ANG ang
#define SCAN_CLOSE_PIX pix
#define SCAN_CLOSE_HAS_PIX has_pix
#define SCAN_CLOSE_SCALE Z->scale[1 + s]
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
    }
    if (code) // one report per ray, whatever the number of records it fails under
        report_failure(code);
}

// (the launch bounds of rt_step_rscan_kernel<true>)
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES) rt_step_rscan_ase_seeds_kernel(const ScanAseSeedsKArg A)
{
#define SCAN_WG_KARG ScanAseSeedsKArg
#define SCAN_WG_NREC (1 + A.set.n_seed) * H.L
#define SCAN_WG_TILES_PER_FETCH FREQ_TILES_PER_FETCH_EMIS
#define SCAN_WG_SET ScanAsePtr
#define SCAN_WG_TILE step_rscan_ase_seeds_tile
#include "rt_step_scan_wg.inc"
#undef SCAN_WG_KARG
#undef SCAN_WG_NREC
#undef SCAN_WG_TILES_PER_FETCH
#undef SCAN_WG_SET
#undef SCAN_WG_TILE
}

} // namespace rt
