// rt_records.h -- the records a step run leaves, as plain numbers.
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
#pragma once

#include <cstddef>

namespace rtr {

// the second pass of a two-kernel run
// (PASS_ASE_SEEDS: an emission plan with ASE seeds, rt_step_ase_seeds.hip -- use_emis with n_seed > 0 and no scan is that and
// nothing else; PASS_SCAN_ASE_SEEDS: the same with the length scan on, rt_step_scan_ase_seeds.hip; PASS_RSCAN: the suffix
// scan of a backward plan, rt_step_rscan.hip -- scan_on with method 1 and no seeds is that and nothing else;
// PASS_RSCAN_ASE_SEEDS: the suffix scan of an emission plan with ASE seeds, rt_step_rscan_ase_seeds.hip)
enum PassKind {
    PASS_FREQ = 0, PASS_SPEC = 1, PASS_STEP = 2, PASS_SEEDS = 3, PASS_PATH = 4, PASS_SCAN = 5, PASS_SCAN_SEEDS = 6, PASS_ASE_SEEDS = 7,
    PASS_SCAN_ASE_SEEDS = 8, PASS_RSCAN = 9, PASS_RSCAN_ASE_SEEDS = 10
};

enum RecordKind { REC_NONE = 0, REC_SEEDS, REC_ASE_SEEDS, REC_SCAN, REC_SCAN_SEEDS, REC_SCAN_ASE_SEEDS, REC_RSCAN, REC_RSCAN_ASE_SEEDS };

struct RecordSet {
    RecordKind kind = REC_NONE; // REC_NONE: one step record in the plan's step buffers (or no step run at all)
    int n_seed      = 0;        // seeds of the set, ASE seeds, seeds of the scan
    int L           = 0;        // lengths of a scan (N - 1)

    bool scan() const { return kind == REC_SCAN || kind == REC_SCAN_SEEDS || ase_scan() || kind == REC_RSCAN; }
    // the whole step record at every n: the ASE curve and one curve per seed, of a length scan or of a suffix scan
    bool ase_scan() const { return kind == REC_SCAN_ASE_SEEDS || kind == REC_RSCAN_ASE_SEEDS; }
    int n_rec() const
    {
        return kind == REC_SEEDS ? n_seed : kind == REC_ASE_SEEDS ? 1 + n_seed : kind == REC_SCAN || kind == REC_RSCAN ? L : kind == REC_SCAN_SEEDS ? n_seed * L :
               ase_scan() ? (1 + n_seed) * L : 0;
    }
    // the block of seed (or ASE record) s and length n, -1 where the set has no such record; a kind without lengths takes
    // no notice of n, a scan without seeds has s = 0 only
    int block(int s, int n = 0) const
    {
        const bool n_ok = n >= 2 && n - 1 <= L;
        switch (kind) {
        case REC_SEEDS: return s >= 0 && s < n_seed ? s : -1;
        case REC_ASE_SEEDS: return s >= 0 && s <= n_seed ? s : -1;
        case REC_SCAN:
        case REC_RSCAN: return s == 0 && n_ok ? n - 2 : -1;
        case REC_SCAN_SEEDS: return s >= 0 && s < n_seed && n_ok ? s * L + n - 2 : -1;
        case REC_SCAN_ASE_SEEDS:
        case REC_RSCAN_ASE_SEEDS: return s >= 0 && s <= n_seed && n_ok ? s * L + n - 2 : -1;
        default: return -1;
        }
    }
    // the record rt_hip_plan_fetch and rt_hip_plan_fetch_step serve
    int primary() const { return scan() ? L - 1 : 0; }
    PassKind pass_kind() const
    {
        return kind == REC_SEEDS ? PASS_SEEDS : kind == REC_ASE_SEEDS ? PASS_ASE_SEEDS : kind == REC_SCAN ? PASS_SCAN : kind == REC_SCAN_SEEDS ? PASS_SCAN_SEEDS :
               kind == REC_SCAN_ASE_SEEDS ? PASS_SCAN_ASE_SEEDS : kind == REC_RSCAN ? PASS_RSCAN : kind == REC_RSCAN_ASE_SEEDS ? PASS_RSCAN_ASE_SEEDS :
               PASS_STEP;
    }
    // bytes per ray of the marks of a checking repeat: one bit per seed in a byte, per length in a 32-bit word, per
    // (seed, length) in a 64-bit word, per (record, length) in four 32-bit words
    size_t bad_word() const { return kind == REC_SCAN || kind == REC_RSCAN ? 4 : kind == REC_SCAN_SEEDS ? 8 : ase_scan() ? 16 : 1; }
};

} // namespace rtr
