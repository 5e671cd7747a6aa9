#pragma once
// rt_step_scan_ase_seeds.hip -- step mode of an EMISSION plan with a length scan AND ASE seeds of the scan
// (rt_hip_plan_set_scan_ase_seeds): the whole per-step record -- the ASE triple and one seeded triple per seed beam -- at
// every plasma length n = 2 .. N from ONE forward march.
//
// The two premises are those of rt_step_ase_seeds.hip and rt_step_scan.hip: the march does not depend on the emission
// switch apart from evl, and the forward run of n lengths is a prefix of the run of N.  The march is the scan march
// unchanged (MODE 3, MARCH_OPT_SCAN); rt_step_scan_ase_seeds_kernel stands where rt_step_scan_kernel stands and leaves
// (1 + n_seed) L records, record (r, j) = block r L + (j - 1) -- a record's curve is contiguous, the ASE curve first:
//   (0, j)       what rt_step_scan_kernel<true> leaves for length j on this plan: the per-slot SF = 0 emission text
//                (ase_step / ase_update, wnan, exact emission honoured), the plan's scale
//   (1 + s, j)   what rt_step_scan_seeds_kernel leaves for (s, j) on a plan of the same problem created with a seed:
//                gain-only, Iv[k] = (f0_s sfk_s[k]) eg_j[k], one exp_tab_vec per length for all seeds, scale scales[s]
// The kernel is made of the fragments of the scan passes: the shell (rt_step_scan_wg.inc), the tile preamble and the
// per-seed factor at the launch ray (rt_step_scan_tile.inc), the state that serves length j (rt_step_scan_state.inc) -- one
// place_ray per length, shared by all records --, the forward walk in its emission form and in its form with a seed set
// (rt_step_scan_walk.inc) and the close of a record (rt_step_scan_close.inc).
//
// Per tile the lengths are taken in chunks of SCAN_ASE_LCH = 2, and per chunk the frequencies are walked TWICE, as the
// SF = 6 instance of rt_step_ase_seeds_kernel does (its HALVES): first the emission recurrence over the slots with the sum
// of record (0, j) per length, then the f64 product sum gl with the sums of (1 + s, j).  One loop with both would hold the
// running Iv, wnan and gl of a batch beside 1 + n_seed sums per length; in two loops the emission half holds two sums and
// the two launch factors, the seed half six sums: 115 VGPRs, no scratch, four waves per SIMD.  Larger chunks spill; four
// lengths for the emission half with two and two for the seed half fit by registers (126) and keep a 48-byte stack frame
// (profiles/scan_ase_seeds_kernel_resources.txt has the alternatives).
// Both halves start at slot 0 per chunk and batch: the slots below the chunk are integrated again without depositing.
// At the end of a chunk, per length: the failure tests of all records, the runs of equal pixel once (rt_wave_runs.inc), then
// per record the I_ang add and the segmented nf scan.  Everything per (record, length) is a register under wave-uniform
// unrolled tests.
//
// F_SKIP (rt_step_ase_seeds.hip): a ray whose sums over the whole N-run are all zero is masked from the ASE records only
// and is live for the seed records; a tile none of whose rays is live for record 0 skips the emission half.  A ray whose
// sums are zero up to some length only is not marked: it adds +0 to the shorter ASE records by arithmetic.
//
// Failures follow the reference run once per (record, length): error -1 at length j puts the ray in no record of that
// length and sets bit 1 in the code of every (r, j); error -2 / -3 under (r, j) removes the ray from (r, j) only.  A failing
// ray is reported once, with the OR of its codes; DevCtl::rec_len_code[r][j - 1] holds the code of (r, j).  The checking
// repeat keeps its two passes; the mark of a ray is one bit per (record, length), bit j - 1 of word r of four 32-bit words
// per ray (FreqHot::bad is an array of such 16-byte marks here), written by the one lane that holds the ray.
#include "rt_step_scan_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int SCAN_ASE_LCH = 2; // lengths per pass over a tile
static_assert(1 + RT_N_SEED_MAX <= 4 && RT_N_SCAN_MAX <= 32, "one mark bit per (record, length) in four 32-bit words per ray");

// the seeds and the scales of the records: what rt_step_scan_ase_seeds_kernel reads beside the blocks of rt_step_scan_kernel
// (through the constant address space, where it is needed)
struct ScanAseSeedsArg {
    int n_seed;
    int pad;
    double scale[1 + RT_N_SEED_MAX]; // of every record's curve (scale[0] is the plan's, FreqHot::scale)
    SeedTabs tabs;
};
static_assert(offsetof(ScanAseSeedsArg, tabs) == 8 + sizeof(double) * (1 + RT_N_SEED_MAX) &&
                  sizeof(ScanAseSeedsArg) == offsetof(ScanAseSeedsArg, tabs) + sizeof(SeedTabs),
              "nesting SeedTabs moves no byte of the argument block");
struct ScanAseSeedsKArg {
    FreqHot hot;
    FreqCold cold;
    ScanArg scan; // out: (1 + n_seed) L blocks, block r L + (j - 1) the record of r (0: ASE, 1 + s: seed s) at length j
    ScanAseSeedsArg set;
};
typedef const RT_CONST_AS ScanAseSeedsArg *ScanAsePtr;

__device__ __forceinline__ void step_scan_ase_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, ScanAsePtr Z, const int n_seed,
                                                         double *lds_iang, double *lds_ev, const double *tab, double *xpose, const unsigned tile,
                                                         const int lane)
{
    constexpr int SF  = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH = SCAN_ASE_LCH;
    constexpr int NS  = RT_N_SEED_MAX;
#define SCAN_TILE_BACKWARD false // the forward method: the scan takes no other
#define SCAN_TILE_MARK unsigned  // four words per ray: word r the lengths of record r
#define SCAN_TILE_HEAD
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_HEAD
#undef SCAN_TILE_BACKWARD
#undef SCAN_TILE_MARK
#define SCAN_TILE_ON_GRID Z->tabs.sf[0]
#define SCAN_TILE_LAUNCH_FACTORS
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_LAUNCH_FACTORS
#undef SCAN_TILE_ON_GRID
#define SCAN_TILE_REC
#include "rt_step_scan_tile.inc"
#undef SCAN_TILE_REC

    unsigned code = 0u; // OR of this ray's codes over records and lengths

    for (int j0 = 0; j0 < L; j0 += LCH) {
        int pix[LCH], ang[LCH];
        double angsum[1 + NS][LCH];
        // bit li: the ray is placed at / carries its seed factors at length j0 + li + 1; bit r LCH + li: the ray is live under /
        // has had a negative Iv under record r at that length
        unsigned placed = 0u, seeded = 0u, live = 0u, neg = 0u;
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            const int j = j0 + li + 1; // the length, 1-based
            pix[li]     = -1;
            ang[li]     = -1;
#pragma unroll
            for (int r = 0; r < 1 + NS; r++)
                angsum[r][li] = 0.0;
            if (j <= L) {
                // the state that serves length j (error -1 whatever the record: out of every record (r, j)); one placement,
                // shared by all records.  Live under record r: not where the checking pass found the ray failing; record 0: not
                // a ray the march marked F_SKIP (the seed records take it)
#define SCAN_STATE_SEG j
#define SCAN_STATE_REPORT(b)                                                                                     \
    _Pragma("unroll") for (int r = 0; r < 1 + NS; r++) if (r <= n_seed) atomicOr(&H.ctl->rec_len_code[r][b], 1u << 1);
#define SCAN_STATE_PLACED                                                                                        \
    placed |= 1u << li;                                                                                          \
    pix[li] = P.pix;                                                                                             \
    ang[li] = P.ang;                                                                                             \
    if (!(flj & F_ESCAPED)) /* (an escaped ray's seed factor is 0, Helper.h:523-533) */                         \
        seeded |= 1u << li;                                                                                      \
    _Pragma("unroll") for (int r = 0; r < 1 + NS; r++) {                                                         \
        if (r <= n_seed) {                                                                                       \
            const unsigned marked = safe_skip ? mark[4u * ridx + (unsigned) r] : 0u;                             \
            if (!((marked >> (j - 1)) & 1u) && !(r == 0 && (fl & F_SKIP)))                                       \
                live |= 1u << (r * LCH + li);                                                                    \
        }                                                                                                        \
    }
#define SCAN_STATE_FORWARD
#include "rt_step_scan_state.inc"
#undef SCAN_STATE_FORWARD
#undef SCAN_STATE_SEG
#undef SCAN_STATE_REPORT
#undef SCAN_STATE_PLACED
            }
            // (one placement after the other, as in rt_step_scan.hip)
            asm volatile("" ::: "memory");
        }
        if (__ballot(placed != 0u) == 0ull)
            continue;
        constexpr unsigned chunk_bits = (1u << LCH) - 1u;
        const bool any0               = __ballot((live & chunk_bits) != 0u) != 0ull; // (else rt_step_scan_kernel skips the chunk)

        const int s_lo = j0 * RT_N_SUB; // the slots below the chunk: integrated again, nothing deposited
#define SCAN_WALK_SUM(r) angsum[r][li]
#define SCAN_WALK_DEPOSITS(r) pix[li] >= 0 && ((live >> (r * LCH + li)) & 1u) != 0u
        // ---- the emission half: records (0, j) of the chunk ----
        if (any0) {
#define SCAN_WALK_EMISSION
#include "rt_step_scan_walk.inc"
#undef SCAN_WALK_EMISSION
        }
        // ---- the seed half: records (1 + s, j) of the chunk, each with its scale ----
#define SCAN_WALK_REC(s) (1 + s)
#define SCAN_WALK_SCALE(r) Z->scale[r]
#define SCAN_WALK_SEEDS
#include "rt_step_scan_walk.inc"
#undef SCAN_WALK_SEEDS
#undef SCAN_WALK_REC
#undef SCAN_WALK_SCALE
#undef SCAN_WALK_SUM
#undef SCAN_WALK_DEPOSITS
        // ---- per length of the chunk: per record the failure test; the runs of equal pixel once; per record the deposit
        // (rt_step_scan_close.inc) ----
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            if (j0 + li < L) {
                const int jb  = j0 + li; // block (within a record's curve) and bit of this length
                const int px  = pix[li];
                const bool dp = px >= 0;
                unsigned failing_r = 0u; // bit r: the ray fails under record r at this length
#pragma unroll
                for (int r = 0; r < 1 + NS; r++) {
                    if (r <= n_seed) {
#define SCAN_CLOSE_SUM angsum[r][li]
#define SCAN_CLOSE_BIT r * LCH + li
#define SCAN_CLOSE_LIVE ((live >> (r * LCH + li)) & 1u)
#define SCAN_CLOSE_CODE H.ctl->rec_len_code[r][jb]
                        // (the lane that holds the ray writes its bits, chunk by chunk: a chunk's lengths are its own)
#define SCAN_CLOSE_MARK                                                                                          \
    if (safe_check)                                                                                              \
        mark[4u * ridx + (unsigned) r] |= 1u << jb;
#define SCAN_CLOSE_FAILS failing_r |= 1u << r;
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
                    for (int r = 0; r < 1 + NS; r++) {
                        if (r <= n_seed) {
                            const bool ok = ((live >> (r * LCH + li)) & 1u) && !((failing_r >> r) & 1u);
#define SCAN_CLOSE_OK ok
#define SCAN_CLOSE_BLOCK r * L + jb
#define SCAN_CLOSE_ANG ang[li]
#define SCAN_CLOSE_PIX px
#define SCAN_CLOSE_SCALE (r == 0 ? H.scale : Z->scale[r])
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
    if (code) // one report per ray, whatever the number of records and lengths it fails at
        report_failure(code);
}

// (the register budget of rt_step_scan_kernel<true>)
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES) rt_step_scan_ase_seeds_kernel(const ScanAseSeedsKArg A)
{
#define SCAN_WG_KARG ScanAseSeedsKArg
#define SCAN_WG_NREC (1 + A.set.n_seed) * H.L
#define SCAN_WG_TILES_PER_FETCH FREQ_TILES_PER_FETCH_EMIS
#define SCAN_WG_SET ScanAsePtr
#define SCAN_WG_TILE step_scan_ase_seeds_tile
#include "rt_step_scan_wg.inc"
#undef SCAN_WG_KARG
#undef SCAN_WG_NREC
#undef SCAN_WG_TILES_PER_FETCH
#undef SCAN_WG_SET
#undef SCAN_WG_TILE
}

} // namespace rt
