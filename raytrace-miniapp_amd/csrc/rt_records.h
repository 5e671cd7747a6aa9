// rt_records.h -- the records a step run leaves and the rows a per-ray spectra run leaves, as plain numbers.
//
// A step run of a seed set, of ASE seeds, of a length scan or of a scan with its seeds leaves several records from one
// march.  They are the blocks of ONE allocation of the plan (rt_hip_plan::rec_dev): n_rec() blocks of E_v | nf | I_ang.
// RecordSet says which blocks a run has and what an index of the C ABI means; rt_run_shape.h builds it from the facts of
// a run (record_set), the plan keeps the one of its last run (rt_runtime.h).  A header of its own because the plan holds
// one, and rt_run_shape.h can only be read behind the kernel files.  No HIP, no plan.
//
//   kind                 blocks          index of the C ABI -> block                    primary()
//   REC_SEEDS            n_seed          seed s -> s                                    0 (seed 0)
//   REC_ASE_SEEDS        1 + n_seed      record r -> r (0: ASE, 1 + s: seed s)          0 (the ASE record)
//   REC_SCAN             L               length n = 2 .. L + 1 -> n - 2                 L - 1 (all N lengths)
//   REC_SCAN_SEEDS       n_seed L        (s, n) -> s L + n - 2; n alone: seed 0         L - 1 (seed 0, all N lengths)
//   REC_SCAN_ASE_SEEDS   (1 + n_seed) L  (r, n) -> r L + n - 2; n alone: the ASE curve  L - 1 (ASE, all N lengths)
//   REC_RSCAN            L               the LAST n lengths, n = 2 .. L + 1 -> n - 2    L - 1 (all N lengths)
//   REC_RSCAN_ASE_SEEDS  (1 + n_seed) L  (r, n) -> r L + n - 2, the LAST n lengths         L - 1 (ASE, all N lengths)
//   REC_RSCAN_SEEDS      n_seed L        (s, n) -> s L + n - 2, the LAST n lengths; n alone: seed 0  L - 1 (seed 0, all N lengths)
//
// The table is code twice below: record_kinds[] holds what tells the kinds apart, one row each, and RecordSet derives every
// column from the row; the static_asserts at the end restate the table at n_seed = 2, L = 3, in range and out of it.  A new
// kind is one row here (and its static_assert), one kernel block in launch_pass (rt_launch.hip) and thin extern "C" callers
// of the shared installer, accessors and loop driver (rt_plan.hip).
#pragma once

#include <cstddef>

namespace rtr {

// the second pass of a two-kernel run
// (PASS_ASE_SEEDS: an emission plan with ASE seeds, rt_step_ase_seeds.hip -- use_emis with n_seed > 0 and no scan is that and
// nothing else; PASS_SCAN_ASE_SEEDS: the same with the length scan on, rt_step_scan_ase_seeds.hip; PASS_RSCAN: the suffix
// scan of a backward plan, rt_step_rscan.hip -- scan_on with method 1 and no seeds is that and nothing else;
// PASS_RSCAN_ASE_SEEDS: the suffix scan of an emission plan with ASE seeds, rt_step_rscan_ase_seeds.hip; PASS_RSCAN_SEEDS:
// the suffix scan of a seeded backward plan with the seeds of the scan, rt_step_rscan_seeds.hip; PASS_SPEC_SCAN: length
// spectra, rt_spec_scan.hip -- per-ray spectra at every length from the scan march, no step record: no RecordKind has it;
// PASS_SPEC_SEEDS / PASS_SPEC_SCAN_SEEDS: spectra mode / length spectra with the seeds of rt_hip_plan_set_spectra_seeds,
// rt_spec_seeds.hip / rt_spec_scan_seeds.hip -- the same per-ray outputs once per seed beam; nothing deposited, no RecordKind;
// PASS_SPEC_ASE_SEEDS: spectra mode of an emission plan with the seeds of rt_hip_plan_set_spectra_ase_seeds, rt_spec_ase_seeds.hip --
// the ASE rows and one block of rows per seed beam; likewise no RecordKind: the step history does not apply;
// PASS_SPEC_SCAN_ASE_SEEDS: length spectra of an emission plan with the seeds of rt_hip_plan_set_length_spectra_ase_seeds,
// rt_spec_scan_ase_seeds.hip -- the ASE curve and one curve per seed beam, a block of rows per (curve, length); no RecordKind)
enum PassKind {
    PASS_FREQ = 0, PASS_SPEC = 1, PASS_STEP = 2, PASS_SEEDS = 3, PASS_PATH = 4, PASS_SCAN = 5, PASS_SCAN_SEEDS = 6, PASS_ASE_SEEDS = 7,
    PASS_SCAN_ASE_SEEDS = 8, PASS_RSCAN = 9, PASS_RSCAN_ASE_SEEDS = 10, PASS_RSCAN_SEEDS = 11, PASS_SPEC_SCAN = 12,
    PASS_SPEC_SEEDS = 13, PASS_SPEC_SCAN_SEEDS = 14, PASS_SPEC_ASE_SEEDS = 15, PASS_SPEC_SCAN_ASE_SEEDS = 16
};

enum RecordKind { REC_NONE = 0, REC_SEEDS, REC_ASE_SEEDS, REC_SCAN, REC_SCAN_SEEDS, REC_SCAN_ASE_SEEDS, REC_RSCAN, REC_RSCAN_ASE_SEEDS,
                  REC_RSCAN_SEEDS };
constexpr int REC_N_KINDS = REC_RSCAN_SEEDS + 1;

// What tells the kinds apart, one row per kind; everything RecordSet says of a kind is derived from its row.
struct RecordKindRow {
    bool lengths;     // one block per length n = 2 .. L + 1 (of every seed or record)
    bool ase;         // a leading ASE record: r = 0 .. n_seed
    bool seeds;       // it carries seeds: s = 0 .. n_seed - 1 (behind the ASE record where there is one)
    bool suffix;      // the suffix form: the lengths are the LAST n of a backward march
    PassKind pass;    // the kernel that leaves the records (rt_launch.hip, launch_pass)
    size_t bad_word;  // bytes per ray of the marks of a checking repeat: one bit per seed in a byte, per length in a 32-bit word,
                      // per (seed, length) in a 64-bit word, per (record, length) in four 32-bit words
    const char *name; // as the messages name the kind ("step kernel of <name>")
    const char *acc;  // its E_v accumulators in the LDS, as the message of a pass that does not fit names them
};
constexpr RecordKindRow record_kinds[REC_N_KINDS] = {
    // lengths ase  seeds  suffix
    { false, false, false, false, PASS_STEP, 1, "a step run", "" },                                             // REC_NONE
    { false, false, true, false, PASS_SEEDS, 1, "a seed set", "per seed" },                                     // REC_SEEDS
    { false, true, true, false, PASS_ASE_SEEDS, 1, "an emission plan with ASE seeds", "for ASE and per seed" }, // REC_ASE_SEEDS
    { true, false, false, false, PASS_SCAN, 4, "a length scan", "per length" },                                 // REC_SCAN
    { true, false, true, false, PASS_SCAN_SEEDS, 8, "a length scan with scan seeds", "per seed and length" },   // REC_SCAN_SEEDS
    { true, true, true, false, PASS_SCAN_ASE_SEEDS, 16, "a length scan with ASE seeds", "per record and length" }, // REC_SCAN_ASE_SEEDS
    { true, false, false, true, PASS_RSCAN, 4, "a suffix scan", "per length" },                                 // REC_RSCAN
    { true, true, true, true, PASS_RSCAN_ASE_SEEDS, 16, "a suffix scan with ASE seeds", "per record and length" }, // REC_RSCAN_ASE_SEEDS
    { true, false, true, true, PASS_RSCAN_SEEDS, 8, "a suffix scan with scan seeds", "per seed and length" },   // REC_RSCAN_SEEDS
};

struct RecordSet {
    RecordKind kind = REC_NONE; // REC_NONE: one step record in the plan's step buffers (or no step run at all)
    int n_seed      = 0;        // seeds of the set, ASE seeds, seeds of the scan
    int L           = 0;        // lengths of a scan (N - 1)

    constexpr const RecordKindRow &row() const { return record_kinds[kind]; }
    constexpr bool scan() const { return row().lengths; }
    // the whole step record at every n: the ASE curve and one curve per seed, of a length scan or of a suffix scan
    constexpr bool ase_scan() const { return row().lengths && row().ase; }
    // values of the first index: the ASE record and the seeds, the seeds, or 0 alone (a scan without seeds)
    constexpr int n_first() const { return row().seeds ? (row().ase ? 1 : 0) + n_seed : 1; }
    constexpr int n_rec() const { return kind == REC_NONE ? 0 : n_first() * (row().lengths ? L : 1); }
    // the block of seed (or ASE record) s and length n, -1 where the set has no such record; a kind without lengths takes
    // no notice of n, a scan without seeds has s = 0 only
    constexpr int block(int s, int n = 0) const
    {
        if (kind == REC_NONE || s < 0 || s >= n_first())
            return -1;
        if (!row().lengths)
            return s;
        return n >= 2 && n - 1 <= L ? s * L + n - 2 : -1;
    }
    // the record rt_hip_plan_fetch and rt_hip_plan_fetch_step serve
    constexpr int primary() const { return scan() ? L - 1 : 0; }
    constexpr PassKind pass_kind() const { return row().pass; }
    constexpr size_t bad_word() const { return row().bad_word; }
};

// ---- the table of the header comment at n_seed = 2, L = 3 (n = 2 .. 4), checked at every compile ------------------------
namespace records_check {
constexpr RecordSet of(RecordKind k) { return RecordSet{ k, 2, 3 }; }
// blocks(k, first, lengths): every (s, n) of s = -1 .. first, n = 1 .. 5 maps as the table says -- inside first x lengths to
// s L + n - 2 (without lengths: to s, whatever n), outside to -1
constexpr bool blocks(RecordKind k, int first, bool lengths)
{
    for (int s = -1; s <= first + 1; s++)
        for (int n = 0; n <= 5; n++) {
            const bool in  = s >= 0 && s < first && (!lengths || (n >= 2 && n <= 4));
            const int want = !in ? -1 : lengths ? s * 3 + n - 2 : s;
            if (of(k).block(s, n) != want)
                return false;
        }
    return of(k).block(0) == (first > 0 && !lengths ? 0 : -1); // (n left out: no length of a scan)
}
constexpr bool is(RecordKind k, int n_rec, int primary, bool scan, bool ase_scan, PassKind pass, size_t bad_word)
{
    return of(k).n_rec() == n_rec && of(k).primary() == primary && of(k).scan() == scan && of(k).ase_scan() == ase_scan &&
           of(k).pass_kind() == pass && of(k).bad_word() == bad_word;
}
static_assert(blocks(REC_NONE, 0, false) && is(REC_NONE, 0, 0, false, false, PASS_STEP, 1), "REC_NONE: no block");
static_assert(blocks(REC_SEEDS, 2, false) && is(REC_SEEDS, 2, 0, false, false, PASS_SEEDS, 1), "REC_SEEDS: seed s -> s");
static_assert(blocks(REC_ASE_SEEDS, 3, false) && is(REC_ASE_SEEDS, 3, 0, false, false, PASS_ASE_SEEDS, 1), "REC_ASE_SEEDS: record r -> r");
static_assert(blocks(REC_SCAN, 1, true) && is(REC_SCAN, 3, 2, true, false, PASS_SCAN, 4), "REC_SCAN: n -> n - 2");
static_assert(blocks(REC_SCAN_SEEDS, 2, true) && is(REC_SCAN_SEEDS, 6, 2, true, false, PASS_SCAN_SEEDS, 8), "REC_SCAN_SEEDS: (s, n) -> s L + n - 2");
static_assert(blocks(REC_SCAN_ASE_SEEDS, 3, true) && is(REC_SCAN_ASE_SEEDS, 9, 2, true, true, PASS_SCAN_ASE_SEEDS, 16),
              "REC_SCAN_ASE_SEEDS: (r, n) -> r L + n - 2");
static_assert(blocks(REC_RSCAN, 1, true) && is(REC_RSCAN, 3, 2, true, false, PASS_RSCAN, 4), "REC_RSCAN: n -> n - 2");
static_assert(blocks(REC_RSCAN_ASE_SEEDS, 3, true) && is(REC_RSCAN_ASE_SEEDS, 9, 2, true, true, PASS_RSCAN_ASE_SEEDS, 16),
              "REC_RSCAN_ASE_SEEDS: (r, n) -> r L + n - 2");
static_assert(blocks(REC_RSCAN_SEEDS, 2, true) && is(REC_RSCAN_SEEDS, 6, 2, true, false, PASS_RSCAN_SEEDS, 8), "REC_RSCAN_SEEDS: (s, n) -> s L + n - 2");
} // namespace records_check

// ---- the rows a per-ray spectra run leaves ---------------------------------------------------------------------------------
// A run of spectra mode or of length spectra leaves, per ray, a spectrum Iv [K], the exit ray ray2 and a code err -- once
// (plain spectra mode), once per seed beam, once per length, or once per (seed beam, length), all from one march.  They are
// the blocks of ONE allocation, Iv [n_blocks()][n_rays][K] | ray2 [n_ray2_blocks()][n_rays] | err [n_blocks()][n_rays]: the
// ray count of the run is the block stride, so it belongs here.  RowSet says which blocks a run has and what an index of the
// C ABI means; rt_run_shape.h builds it from the facts of a run (row_set), the plan keeps the one of its last run
// (rt_runtime.h), and rt_plan.hip serves the rows by it.
//
//   kind                 blocks of Iv / err   blocks of ray2   index of the C ABI -> block
//   ROWS_NONE            0                    0                none (no spectra run)
//   ROWS_SPEC            1                    1                -> 0
//   ROWS_SPEC_SEEDS      n_seed               1                seed s -> s
//   ROWS_SPEC_ASE_SEEDS  1 + n_seed           1                block r -> r (0: ASE, 1 + s: seed s)
//   ROWS_LSPEC           L                    L                length n = 2 .. L + 1 -> n - 2
//   ROWS_LSPEC_SEEDS     n_seed L             L                (s, n) -> s L + n - 2; n alone: seed 0
//   ROWS_LSPEC_ASE_SEEDS (1 + n_seed) L       L                (r, n) -> r L + n - 2 (0: ASE, 1 + s: seed s); n alone: the ASE curve
//
// As above the table is code twice: row_kinds[] holds what tells the kinds apart, RowSet derives every column from the row,
// and the static_asserts restate the table at n_seed = 2, L = 3.  A new kind is one row here (and its static_assert), one
// kernel block in launch_pass (rt_launch.hip) and thin extern "C" callers of the shared accessors (rt_plan.hip).
enum RowKind { ROWS_NONE = 0, ROWS_SPEC, ROWS_SPEC_SEEDS, ROWS_SPEC_ASE_SEEDS, ROWS_LSPEC, ROWS_LSPEC_SEEDS, ROWS_LSPEC_ASE_SEEDS };
constexpr int ROWS_N_KINDS = ROWS_LSPEC_ASE_SEEDS + 1;

struct RowKindRow {
    bool lengths;     // one block per length n = 2 .. L + 1 (of every seed), of ray2 as well
    bool ase;         // a leading block of ASE rows: r = 0 .. n_seed
    bool seeds;       // it carries seeds: s = 0 .. n_seed - 1 (behind the ASE block where there is one)
    PassKind pass;    // the kernel that leaves the rows (rt_launch.hip, launch_pass)
    const char *mode; // the mode, as the message of a pass that does not fit names its kernel
    const char *who;  // the kernel, as the messages of launch_pass name it
};
constexpr RowKindRow row_kinds[ROWS_N_KINDS] = {
    // lengths ase  seeds
    { false, false, false, PASS_FREQ, "", "" },                                                                   // ROWS_NONE
    { false, false, false, PASS_SPEC, "spectra kernel", "spectra kernel" },                                       // ROWS_SPEC
    { false, false, true, PASS_SPEC_SEEDS, "spectra kernel", "spectra kernel with seeds" },                       // ROWS_SPEC_SEEDS
    { false, true, true, PASS_SPEC_ASE_SEEDS, "spectra kernel", "spectra kernel with ASE seeds" },                // ROWS_SPEC_ASE_SEEDS
    { true, false, false, PASS_SPEC_SCAN, "length spectra kernel", "length spectra kernel" },                     // ROWS_LSPEC
    { true, false, true, PASS_SPEC_SCAN_SEEDS, "length spectra kernel", "length spectra kernel with seeds" },     // ROWS_LSPEC_SEEDS
    { true, true, true, PASS_SPEC_SCAN_ASE_SEEDS, "length spectra kernel", "length spectra kernel with ASE seeds" }, // ROWS_LSPEC_ASE_SEEDS
};
// the passes that leave per-ray spectra: the pass of some row
constexpr bool spectra_pass(PassKind kind)
{
    for (int k = ROWS_SPEC; k < ROWS_N_KINDS; k++)
        if (row_kinds[k].pass == kind)
            return true;
    return false;
}

struct RowSet {
    RowKind kind  = ROWS_NONE; // ROWS_NONE: no spectra run (an image, a step run, the path tracer, or no run at all)
    int n_seed    = 0;         // seeds of rt_hip_plan_set_spectra_seeds / rt_hip_plan_set_spectra_ase_seeds / rt_hip_plan_set_length_spectra_ase_seeds
    int L         = 0;         // lengths of length spectra (N - 1)
    size_t n_rays = 0;         // rays of the run: the stride from block to block, in rows

    constexpr const RowKindRow &row() const { return row_kinds[kind]; }
    constexpr bool any() const { return kind != ROWS_NONE; }
    constexpr bool lengths() const { return row().lengths; }
    // values of the first index: the ASE block and the seeds, the seeds, or 0 alone
    constexpr int n_first() const { return row().seeds ? (row().ase ? 1 : 0) + n_seed : 1; }
    constexpr int n_blocks() const { return any() ? n_first() * (row().lengths ? L : 1) : 0; }
    constexpr int n_ray2_blocks() const { return any() ? (row().lengths ? L : 1) : 0; }
    // the block of Iv and err of seed (or block) s and length n, -1 where the run left no such rows; a kind without lengths
    // takes no notice of n, a kind without seeds has s = 0 only
    constexpr int block(int s, int n = 0) const
    {
        if (!any() || s < 0 || s >= n_first())
            return -1;
        if (!row().lengths)
            return s;
        return n >= 2 && n - 1 <= L ? s * L + n - 2 : -1;
    }
    // ... and the block of ray2, which does not depend on the seed
    constexpr int ray2_block(int n = 0) const { return block(0, n); }
    constexpr PassKind pass_kind() const { return row().pass; }
};

// ---- that table at n_seed = 2, L = 3 (n = 2 .. 4) and 70 rays, checked at every compile ----------------------------------
namespace rows_check {
constexpr RowSet of(RowKind k) { return RowSet{ k, 2, 3, 70 }; }
constexpr bool blocks(RowKind k, int first, bool lengths)
{
    for (int s = -1; s <= first + 1; s++)
        for (int n = 0; n <= 5; n++) {
            const bool in_n = !lengths || (n >= 2 && n <= 4), in = s >= 0 && s < first && in_n;
            if (of(k).block(s, n) != (!in ? -1 : lengths ? s * 3 + n - 2 : s))
                return false;
            if (of(k).ray2_block(n) != (first == 0 || !in_n ? -1 : lengths ? n - 2 : 0))
                return false;
        }
    return true;
}
constexpr bool is(RowKind k, int n_blocks, int n_ray2_blocks, bool lengths, PassKind pass)
{
    return of(k).n_blocks() == n_blocks && of(k).n_ray2_blocks() == n_ray2_blocks && of(k).lengths() == lengths && of(k).pass_kind() == pass &&
           spectra_pass(pass) == (k != ROWS_NONE);
}
static_assert(blocks(ROWS_NONE, 0, false) && is(ROWS_NONE, 0, 0, false, PASS_FREQ), "ROWS_NONE: no block");
static_assert(blocks(ROWS_SPEC, 1, false) && is(ROWS_SPEC, 1, 1, false, PASS_SPEC), "ROWS_SPEC: -> 0");
static_assert(blocks(ROWS_SPEC_SEEDS, 2, false) && is(ROWS_SPEC_SEEDS, 2, 1, false, PASS_SPEC_SEEDS), "ROWS_SPEC_SEEDS: seed s -> s");
static_assert(blocks(ROWS_SPEC_ASE_SEEDS, 3, false) && is(ROWS_SPEC_ASE_SEEDS, 3, 1, false, PASS_SPEC_ASE_SEEDS), "ROWS_SPEC_ASE_SEEDS: block r -> r");
static_assert(blocks(ROWS_LSPEC, 1, true) && is(ROWS_LSPEC, 3, 3, true, PASS_SPEC_SCAN), "ROWS_LSPEC: n -> n - 2");
static_assert(blocks(ROWS_LSPEC_SEEDS, 2, true) && is(ROWS_LSPEC_SEEDS, 6, 3, true, PASS_SPEC_SCAN_SEEDS), "ROWS_LSPEC_SEEDS: (s, n) -> s L + n - 2");
static_assert(blocks(ROWS_LSPEC_ASE_SEEDS, 3, true) && is(ROWS_LSPEC_ASE_SEEDS, 9, 3, true, PASS_SPEC_SCAN_ASE_SEEDS),
              "ROWS_LSPEC_ASE_SEEDS: (r, n) -> r L + n - 2");
static_assert(!spectra_pass(PASS_STEP) && !spectra_pass(PASS_PATH) && !spectra_pass(PASS_SCAN_SEEDS), "the step passes leave no rows");
} // namespace rows_check

} // namespace rtr
