// rt_run_shape.h -- what a run looks like on the device, decided from plain numbers.
//
// Included by rt_launch.hip alone, behind the kernel files (it needs their constexpr sizes).  Everything here is pure: no
// HIP call, no look at the plan -- and the environment is touched by read_tuning() and nothing else.  plan_launch_run
// fills a RunFacts from the plan, reads the Tuning once, calls run_shape and enqueues what it says; the second pass gets
// its numbers from pass_shape.  rt_hip_debug_run_shape hands the same functions to a test that has no device.
#pragma once

#include "rt_records.h"

#include <cstdlib>
#include <cstring>
#include <functional>

namespace rtr {

// ---- what the decision needs to know of a plan ---------------------------------------------------------------------
struct RunFacts {
    int cu_count              = 0;
    size_t lds_limit          = 0;
    unsigned long long n_rays = 0;
    unsigned n_tiles          = 0;
    size_t blob_bytes         = 0;
    int K = 0, Kp = 0, L = 0;
    size_t n_iang             = 0;
    int rays_per_pixel        = 0; // rays.nga * rays.ngb
    int n_seed                = 0;
    float c_h3                = 0.0f;
    int march_prune           = 1;
    int method                = 0;
    unsigned safe = 0, debug = 0;
    bool use_emis = false, own_cells = false, exclusive = false, path_on = false, spectra_on = false, step_on = false,
         step_one_launch = false, probe_on = false, has_ray_list = false, host_rays = false, tables_bounded = false,
         ntest_proven = false, gv_has_nan = false;
    // a length scan (rt_hip_plan_enable_length_scan): one step record per length from one forward march; with method == 1
    // the suffix scan (rt_hip_plan_enable_suffix_scan): one record per run of the last n lengths from one backward march
    bool scan_on = false;
    // length spectra (rt_hip_plan_enable_length_spectra): per-ray spectra at every length from the same scan march, forward
    // or backward by the method; a mode of its own, never together with step_on, spectra_on or scan_on
    bool length_spectra_on = false;
    bool scan_march() const { return scan_on || length_spectra_on; } // the run takes the scan instance of the march
    bool rscan() const { return scan_march() && method == 1; }
    bool s6() const { return L * RT_N_SUB == 6; } // N = 3, the shipped inputs: the instances with SF = 6
};

// ---- every knob of the launch --------------------------------------------------------------------------------------
// A knob whose default (or upper bound) is only known inside the decision is kept as read, KNOB_UNSET where the
// environment does not name it (or names junk), and resolved by knob() where it applies.
constexpr unsigned KNOB_UNSET = ~0u;
inline unsigned knob(unsigned k, unsigned def, unsigned hi = ~0u) { return k == KNOB_UNSET ? def : (k > hi ? hi : k); }

struct Tuning {
    bool march_global; // RT_HIP_MARCH=global: the global-table march whatever fits
    bool march_ieee;   // RT_HIP_MARCH_IEEE set at all: the full IEEE division sequences (rt_math.h, fdiv_nr)
    unsigned upload_slices; // RT_HIP_UPLOAD_SLICES 1 ... 8 (knob; host ray lists only)
    unsigned fused;         // RT_HIP_FUSED: 2 keeps the two kernels
    unsigned fused_seed;    // RT_HIP_FUSED_SEED=1: the gain-only mode on a ray grid as one launch (run_shape says why not)
    unsigned march_threads; // RT_HIP_MARCH_THREADS 64 ... 1024 (256 with global tables), whole waves (knob; occupancy experiments)
    // RT_HIP_MARCH_MODE: gain-only, forward: only the method at compile time -- MODE 3, -0.7 %; with the emission switch
    // fixed as well, or alone, the same source compiles to a march that is 5 - 9 % SLOWER: 2 / 4 / 0 to see it
    unsigned march_mode;
    unsigned march_chunk;   // RT_HIP_MARCH_CHUNK 1 ... 4096 (knob)
    // RT_HIP_MARCH_PARK: lanes that must wait for block [A] of the march before it runs (swept 1 ... 40 on the 6.4 M-ray
    // stand-in: 2.36 ms at 1, flat optimum 2.12 ms at 8 ... 24, 2.63 ms at 40)
    unsigned march_park;
    unsigned march_spin_limit; // RT_HIP_MARCH_SPIN_LIMIT (tests lower it)
    // The chunks at the end of the ray list that only the oldest wave of every SIMD takes (rt_march.hip, "The end of a
    // launch"): about as many rays as those waves march in one drain period, RT_HIP_LATE_X10 tenths of a ray per lane of
    // theirs (0: no such zone) -- RT_HIP_LATE2_X10 for the march as a kernel of its own (60: seed_small -0.8 %, stand-in as
    // two kernels -1.5 %, its 8-rank shard -6 %) --, at most RT_HIP_LATE_CAP per cent of the launch (20: swept 8 ... 35 on
    // the 8- and 16-rank shards and ASE_small.dat, profiles/r05_fused_end.txt).
    unsigned late_x10, late2_x10, late_waves, late_cap;
    unsigned fused_rows;      // RT_HIP_FUSED_ROWS: gain-only, rows of the per-wave row cache (a seeded tile holds ~7 pixels)
    unsigned fused_nodes;     // RT_HIP_FUSED_NODES 0 ... 4096 (knob)
    unsigned fused_split;     // RT_HIP_FUSED_SPLIT = 2: never, 3: every tile (tests)
    unsigned fused_consumers; // RT_HIP_FUSED_CONSUMERS 0 ... waves - 1 (knob)
    unsigned fused_consumers_first; // RT_HIP_FUSED_CONSUMERS_FIRST
    // RT_HIP_FREQ_WG_WAVES.  (exclusive mode: while its flush wrote 8 bytes per lane with a pixel look-up per store, 12
    // waves per CU ran 3.6 % faster than 16; with the regular-tile flush of 16-byte stores 16 waves win -- 22.15 against
    // 23.0 ms on the 4096^2 x 512 image, tools/config5_waves.py)
    unsigned freq_wg_waves;
    unsigned freq_min_rows; // RT_HIP_FREQ_MIN_ROWS: seeded tiles hold ~7 pixels
    unsigned freq_wgs;      // RT_HIP_FREQ_WGS 1 ... 16 (knob; tuning override)
    // RT_HIP_STEP_SERIAL=1: every step pass (step, seed set, length scan, scan seeds, ASE seeds, scan ASE seeds, suffix ASE seeds, suffix seeds) as ONE work-group of ONE wave.  The
    // passes add with f64 atomics in the order in which waves arrive, so two runs of the same rays differ in the last bits;
    // one wave takes the tiles in a fixed order and its sums are the same doubles run after run -- for comparisons bit for
    // bit (tests), at the pace of one wave.  The one-launch step run is not affected.
    unsigned step_serial;
};

// The only place of rt_launch.hip that touches the environment; once per run (and per checking repeat), so that a
// process that changes a knob between two runs sees it.
inline Tuning read_tuning()
{
    Tuning t;
    const char *force       = getenv("RT_HIP_MARCH");
    t.march_global          = force && strcmp(force, "global") == 0;
    t.march_ieee            = getenv("RT_HIP_MARCH_IEEE") != nullptr;
    t.upload_slices         = env_unsigned("RT_HIP_UPLOAD_SLICES", KNOB_UNSET, 1, 8);
    t.fused                 = env_unsigned("RT_HIP_FUSED", 1, 1, 2);
    t.fused_seed            = env_unsigned("RT_HIP_FUSED_SEED", 0, 0, 1);
    t.march_threads         = env_unsigned("RT_HIP_MARCH_THREADS", KNOB_UNSET, 64, 1024);
    t.march_mode            = env_unsigned("RT_HIP_MARCH_MODE", 3, 0, 4);
    t.march_chunk           = env_unsigned("RT_HIP_MARCH_CHUNK", KNOB_UNSET, 1, 4096);
    t.march_park            = env_unsigned("RT_HIP_MARCH_PARK", 12, 1, 64);
    t.march_spin_limit      = env_unsigned("RT_HIP_MARCH_SPIN_LIMIT", 1u << 24, 1024, 0x7fffffffu);
    t.late_x10              = env_unsigned("RT_HIP_LATE_X10", 32, 0, 1000);
    t.late2_x10             = env_unsigned("RT_HIP_LATE2_X10", 60, 0, 1000);
    t.late_waves            = env_unsigned("RT_HIP_LATE_WAVES", 4, 0, 16);
    t.late_cap              = env_unsigned("RT_HIP_LATE_CAP", 20, 0, 100);
    t.fused_rows            = env_unsigned("RT_HIP_FUSED_ROWS", 7, 4, 16);
    t.fused_nodes           = env_unsigned("RT_HIP_FUSED_NODES", KNOB_UNSET, 0, 4096);
    t.fused_split           = env_unsigned("RT_HIP_FUSED_SPLIT", 1, 1, 3);
    t.fused_consumers       = env_unsigned("RT_HIP_FUSED_CONSUMERS", KNOB_UNSET, 0, 4096);
    t.fused_consumers_first = env_unsigned("RT_HIP_FUSED_CONSUMERS_FIRST", 0, 0, 1);
    t.freq_wg_waves         = env_unsigned("RT_HIP_FREQ_WG_WAVES", (unsigned) rt::FREQ_WG_WAVES, 1, (unsigned) rt::FREQ_WG_WAVES);
    t.freq_min_rows         = env_unsigned("RT_HIP_FREQ_MIN_ROWS", 7, 0, 16);
    t.freq_wgs              = env_unsigned("RT_HIP_FREQ_WGS", KNOB_UNSET, 1, 16);
    t.step_serial           = env_unsigned("RT_HIP_STEP_SERIAL", 0, 0, 1);
    return t;
}

// ---- small rules used more than once -------------------------------------------------------------------------------
// one work-group per CU, fewer where the work does not fill them
inline unsigned one_wg_per_cu(unsigned long long items, unsigned per_wg, int cu_count)
{
    const unsigned long long want = (items + per_wg - 1) / per_wg;
    return (unsigned) (want < (unsigned long long) cu_count ? want : (unsigned long long) cu_count);
}
// FreqHot::fetch_shift: ceil(log2(2 x waves of the grid))
inline unsigned fetch_shift_of(unsigned long long grid_waves)
{
    unsigned sh = 0;
    while ((1ull << sh) < 2ull * grid_waves)
        sh++;
    return sh;
}
// rays reserved per counter fetch of a march launch over `rays` rays: big enough to amortise the atomic, small enough that
// the last chunks balance (about 8 chunks per wave), within 64 ... 192 -- swept on the stand-in and on its strong-scaling
// shards (tools/shard_sweep2.py): a whole 64-ray refill per fetch is the least that pays (798 K rays: 0.88 ms at 16, 0.55
// at 32, 0.44 at 64, 0.60 at 96), 64 ... 192 is flat at 6.4 M rays (2.02 ms; 2.66 at 32, 2.05 at 256)
inline unsigned march_chunk(unsigned long long rays, unsigned grid, unsigned bthr)
{
    unsigned long long ch = grid ? rays / ((unsigned long long) grid * (bthr / 64) * 8) : 64;
    ch                    = ch < 64 ? 64 : (ch > 192 ? 192 : ch);
    return (unsigned) ((ch + 15) / 16 * 16);
}

// ---- the run -------------------------------------------------------------------------------------------------------
enum RunKind { RUN_TWO_KERNELS = 0, RUN_IMAGE_ONE_LAUNCH = 1, RUN_STEP_ONE_LAUNCH = 2 };

struct RunShape {
    bool lds_tab      = false; // the march tables in LDS (else the global-table march)
    unsigned n_launch = 1;     // march launches = upload slices of a host ray list
    RunKind kind      = RUN_TWO_KERNELS;
    // the march (of a one-launch run: its march phase)
    unsigned bthr = 0;
    int mode = 0, opt = 0, last_march_inst = 0;
    bool bounded = false;
    size_t mlds  = 0;
    unsigned grid = 0, chunk = 0, park = 0, spin_limit = 0, no_skip = 0;
    unsigned late_first = 0, late_waves = 0, late_chunks = 0;
    bool occupancy_asked = false;
    // a one-launch run
    bool emis = false;
    int maxq = 0, nslot = 0;
    rt::FusedLay lay = {};
    size_t flds = 0, tile_links = 0;
    unsigned fgrid = 0, fetch_shift = 0;
};

// work-groups per CU the device would keep resident of the march instance `s` names, with s.bthr threads and s.mlds bytes
// of LDS (hipOccupancyMaxActiveBlocksPerMultiprocessor, or a number that stands for it)
using Occupancy = std::function<int(const RunShape &s)>;

// the late zone of a launch of `n_rays` rays in chunks of s.chunk on `grid` work-groups (Tuning says what it is)
inline void late_zone(RunShape &s, const Tuning &t, unsigned long long n_rays, unsigned grid, unsigned waves_per_wg, unsigned first_marching_wave,
                      unsigned x10)
{
    // (the waves that take the late chunks must be waves that march: waves_per_wg counts the marching waves,
    // first_marching_wave is where they start inside the work-group)
    s.late_first  = first_marching_wave;
    s.late_waves  = t.late_waves < waves_per_wg ? t.late_waves : waves_per_wg;
    s.late_chunks = 0;
    if (x10 == 0 || s.late_waves == 0 || s.chunk == 0)
        return;
    unsigned long long rays      = (unsigned long long) grid * s.late_waves * 64ull * x10 / 10ull;
    const unsigned long long cap = n_rays * t.late_cap / 100ull; // (per cent of the launch)
    rays                         = rays > cap ? cap : rays;
    s.late_chunks                = (unsigned) (rays / s.chunk);
}

// The layout of a one-launch run in LDS (rt_fused.hip, rt_fused_step.hip) and whether it fits; fills s.maxq, s.nslot,
// s.lay, s.flds on the way.
inline bool one_launch_fits(RunShape &s, const RunFacts &f, const Tuning &t, bool step)
{
    const unsigned nw = s.bthr / 64;
    const bool emis   = s.emis;
    // doubles per wave: transposition rows + window totals of the few-runs deposit for 2 pixel runs per tile (a pixel
    // has at least 64 rays) or 3, no row cache
    s.maxq  = emis && f.rays_per_pixel >= 64 ? 2 : 3;
    // gain-only: rows of the per-wave row cache (a seeded tile holds ~7 pixels; fewer than 4 rows is not worth having)
    s.nslot = emis ? 0 : (int) t.fused_rows;
    size_t per_wave = (size_t) rt::fused_wave_doubles(s.maxq) + (size_t) s.nslot * (size_t) rt::freq_row_stride(f.Kp);
    if (step) // the transposition rows of the wave sum, nothing else (rt_step.hip)
        per_wave = (size_t) 4 * rt::XP_ROW;
    rt::FusedLay &lay = s.lay;
    lay.off_exp  = (unsigned) align_up(f.blob_bytes, 16);
    lay.off_iang = lay.off_exp + 2u * rt::EXP_TAB * (unsigned) sizeof(double);
    lay.off_ctl  = lay.off_iang + (unsigned) (((f.n_iang + 1) & ~(size_t) 1) * sizeof(double));
    if (step) // E_v [Kp] of the work-group behind the histogram: beside the tables, never under an overlaid buffer
        lay.off_ctl = lay.off_iang + rt::fused_step_ev_off((int) f.n_iang) + (unsigned) ((size_t) f.Kp * sizeof(double));
    lay.off_rem   = lay.off_ctl + 16u;
    lay.off_nodes = lay.off_rem + nw * 32u * (unsigned) sizeof(unsigned);
    // nodes of the work-group's tile list in LDS: room for twice a work-group's share of the entries (a tile is one
    // entry, a split tile four; a work-group that marches faster owes more), within 64 ... 1024; the surplus of a
    // work-group that pushes more takes the global links
    {
        const unsigned long long wgs = one_wg_per_cu(f.n_rays, s.bthr, f.cu_count);
        unsigned long long cap       = wgs ? 2ull * ((unsigned long long) f.n_tiles / wgs + 1) + 32 : 64;
        cap                          = cap < 64 ? 64 : (cap > 1024 ? 1024 : cap);
        if (!emis) // (LDS is what the row caches are short of; the consumers keep the list short)
            cap = cap > 256 ? 256 : cap;
        lay.node_cap = knob(t.fused_nodes, (unsigned) cap);
    }
    lay.off_buf = (unsigned) align_up(lay.off_nodes + lay.node_cap * 2u * (unsigned) sizeof(unsigned), 16);
    size_t room = f.lds_limit > lay.off_buf ? (f.lds_limit - lay.off_buf) / (per_wave * sizeof(double)) : 0;
    if (!emis && room < 5 && s.nslot > 5) { // one more buffer beside the tables is worth two rows of each cache
        s.nslot  = 5;
        per_wave = (size_t) rt::fused_wave_doubles(s.maxq) + (size_t) s.nslot * (size_t) rt::freq_row_stride(f.Kp);
        room     = f.lds_limit > lay.off_buf ? (f.lds_limit - lay.off_buf) / (per_wave * sizeof(double)) : 0;
    }
    lay.per_wave = (unsigned) per_wave;
    lay.n_free   = (unsigned) (room < nw ? room : nw);
    s.flds       = (size_t) lay.off_buf + (size_t) lay.n_free * per_wave * sizeof(double);
    // emission: at least half the buffers beside the tables (the others overlay them once the march is over);
    // gain-only: at least three, and they are the consumers'
    return (emis ? 2 * lay.n_free >= nw : (lay.n_free >= 3 && nw >= 8)) && (size_t) (nw - lay.n_free) * per_wave * sizeof(double) <= f.blob_bytes;
}

inline RunShape run_shape(const RunFacts &f, const Tuning &t, const Occupancy &occupancy)
{
    RunShape s;
    // march, LDS variant: the whole march blob in LDS, one work-group of up to 1024 threads per CU;
    // global variant (persistent 256-thread work-groups) when the blob does not fit (RT_HIP_MARCH=global forces it)
    s.lds_tab = f.blob_bytes + 8 * 1024 <= f.lds_limit && !t.march_global;
    // A run is one march launch -- or three, when the ray list is still on the host
    // (rt_hip_image_loop): the list crosses PCIe in slices, each with a synchronous copy (the fast
    // pageable path, ~35 GB/s; asynchronous copies of pageable memory reach a third of that), and
    // the march of a slice runs on image_loop's non-blocking queue while the host copies the next
    // one (16 B/ray: 102 MB, ~3 ms for the 6.4 M-ray case; swept: 3 slices 5.8 ms, 1 slice 6.9, 8 slices 7.3).
    s.n_launch = (f.host_rays && f.n_rays >= (2ull << 20)) ? 3u : 1u;
    if (f.host_rays)
        s.n_launch = knob(t.upload_slices, s.n_launch);
    // ---- the whole path in ONE launch (rt_fused.hip) where it applies: emission mode on the beam's own ray grid
    // with at least 32 rays per pixel (a 64-ray tile then spans at most three pixels: the few-runs deposit, which
    // needs no row cache), tables in LDS, nothing that wants the march records to itself (probe, path tracer,
    // the checking repeat, profiling switches), and room in LDS for the frequency pass beside the tables
    // (The gain-only mode -- a seed, forward method -- on a ray grid can run as one launch as well: its frequency pass needs a
    // row cache per wave, so only the handful of waves whose buffers fit beside the march tables run it during the march
    // (one_launch_fits).  Built and measured in round 5, profiles/r05_seed_fused_ab.txt: seed_small.dat 3.28 against
    // 3.33 ms with four such waves, twice the rays 5.97 against 5.93 ms -- a wash, because what the one launch buys is the
    // idle end of the march, which is a fifth of a 0.5 ms launch and a hundredth of a 6 ms one, and what it costs is five
    // of sixteen waves marching less.  Two kernels stay the rule for this mode; RT_HIP_FUSED_SEED=1 takes the one launch.)
    const bool iang_fits  = f.n_iang * sizeof(double) <= 32 * 1024;
    const bool fused_emis = f.use_emis && f.method == 1 && f.own_cells && f.rays_per_pixel >= 32;
    const bool fused_gain = !f.use_emis && !f.has_ray_list && t.fused_seed == 1;
    const bool fused_cand = s.lds_tab && s.n_launch == 1 && f.n_rays > 0 && !f.path_on && !f.spectra_on && !f.length_spectra_on && !f.step_on && !f.probe_on && f.debug == 0 &&
                            (fused_emis || fused_gain) && !f.exclusive && f.safe == 0 && iang_fits && t.fused == 1;
    // ---- step mode in ONE launch (rt_fused_step.hip), where the caller has asked for it (rt_hip_plan_set_step_one_launch):
    // the conditions of the emission run above without those that exist for the few-runs image deposit only -- the step
    // pass writes no image, so neither 32 rays per pixel nor "a tile spans at most three pixels" is asked for.  Ray lists,
    // seeded plans, seed sets, the exclusive mode (its plain stores into nf must not meet a split tile) and tables that
    // leave no room keep the two kernels.
    const bool step_cand = f.step_on && f.step_one_launch && s.lds_tab && s.n_launch == 1 && f.n_rays > 0 && f.use_emis && f.method == 1 &&
                           f.own_cells && !f.probe_on && !f.path_on && !f.spectra_on && f.debug == 0 && f.safe == 0 && !f.exclusive &&
                           f.n_seed == 0 && !f.scan_on && iang_fits && t.fused == 1;
    s.bthr = s.lds_tab ? 1024u : 256u;
    if (s.lds_tab && !fused_cand && !step_cand) {
        // Few rays per lane leave the persistent lanes waiting for the longest ray of a short
        // queue: below about three rays per lane, fewer and busier lanes win (ASE_small, 399 000
        // rays on 256 CUs: 0.65 ms with 1024 threads per CU, 0.44 ms with 512; 8 waves per CU is
        // the least that still hides latency).
        const unsigned long long per_cu_rays = f.cu_count ? f.n_rays / (unsigned long long) f.cu_count : 0;
        // (tools/shard_threads.py on pixel-column shards of the stand-in: 3117 rays per CU 0.461 ms with 768 threads,
        // 0.472 with 1024; 4156 per CU: equal; 1558 per CU: 0.376 ms with 512, 0.432 with 1024)
        s.bthr = per_cu_rays >= 4ull * 1024 ? 1024u : (per_cu_rays >= 2560ull ? 768u : 512u);
    }
    // (the one-launch run always takes sixteen waves per CU: a quarter of them run the frequency pass from the start and
    // the end of the ray list is kept for the oldest wave of every SIMD, see below -- with those two the full
    // work-group wins at every size measured, 399 K rays ... 6.4 M, profiles/r05_fused_end.txt)
    s.bthr = knob(t.march_threads, s.bthr, s.lds_tab ? 1024 : 256) / 64 * 64;
    s.mlds = s.lds_tab ? f.blob_bytes : 0;
    // the integrator's divisions without range bookkeeping where the tables and the step factor allow it
    // (rt_math.h, fdiv_nr; RT_HIP_MARCH_IEEE=1 forces the full IEEE sequences)
    s.bounded = f.tables_bounded && f.c_h3 >= 1e-8f && !t.march_ieee;
    // (the instance with method and emission switch fixed at compile time for the emission / backward pair, rt_march.hip
    // MODE: the one-launch run -2.1 % with it; profiles/r05_loop_head.txt)
    s.mode = (f.use_emis && f.method == 1 && !f.path_on) ? 1 : 0;
    if (!f.use_emis && f.method == 2 && !f.path_on)
        s.mode = (int) t.march_mode;
    // (the two shortcuts of block [C], rt_march.hip OPT: BOUNDED instances whose tables allow the proof of the |n - n0|
    // test -- every shipped one; other tables keep the old instance, as RT_HIP_MARCH_PRUNE=0 at plan creation does.
    // The branch round the divisions of h2 and h4 pays where the waves compete for issue slots and costs where a
    // launch is a few rays per lane -- measured, profiles/step_prune_ab.txt: 24.9 K rays per CU -2.0 %, 3.1 K a wash,
    // 1.6 K +1 ... 2 %, nothing in between -- so it is taken from 8 K rays per CU and launch; RT_HIP_MARCH_PRUNE=2
    // takes it at every size, for the tests)
    const unsigned long long launch_rays = f.n_rays / s.n_launch;
    const bool prune_h24 = f.march_prune == 2 || (f.cu_count && launch_rays / (unsigned long long) f.cu_count >= 8192ull);
    s.opt = (s.bounded && f.march_prune && f.ntest_proven) ? (rt::MARCH_OPT_PRUNE | rt::MARCH_OPT_NO_NTEST | (prune_h24 ? rt::MARCH_OPT_PRUNE_H24 : 0)) : 0;
    // (a length scan: the instance that stores the boundary states, rt_march.hip MARCH_OPT_SCAN -- forward method at compile
    // time, the emission switch as DevParams says, no pruning; with bounded and unbounded tables, in LDS or not)
    // (the suffix scan: the same stores from the backward march -- MODE 1, backward and emission at compile time, for an
    // emission plan, MODE 0 for a seeded one)
    // (length spectra take the same instances: the march does not know which pass reads its boundary states)
    if (f.scan_march()) {
        s.mode = f.rscan() ? (f.use_emis ? 1 : 0) : 3;
        s.opt  = rt::MARCH_OPT_SCAN;
    }
    s.last_march_inst = (s.bounded ? 1 : 0) | (s.opt << 1);
    // one work-group per CU: the tables take more than half of the LDS... or the work-group all wave slots
    int per_cu = 1;
    if (!s.lds_tab || (2 * s.mlds + 1024 <= f.lds_limit && s.bthr <= 512)) {
        s.occupancy_asked = true;
        per_cu            = occupancy(s);
    }
    if (per_cu < 1)
        per_cu = 1;
    const unsigned long long want = ((unsigned long long) f.n_rays + s.bthr - 1) / s.bthr;
    const unsigned long long cap  = (unsigned long long) f.cu_count * (unsigned) per_cu;
    s.grid       = (unsigned) (want < cap ? want : cap);
    s.chunk      = knob(t.march_chunk, march_chunk(f.n_rays, s.grid, s.bthr));
    s.park       = t.march_park;
    s.spin_limit = t.march_spin_limit;
    s.no_skip    = f.gv_has_nan ? 1u : 0u; // the CPU loop multiplies 0 * gv[row 0] for sub-segments a ray never entered
    s.emis       = f.use_emis;
    if ((fused_cand || step_cand) && s.grid > 0 && one_launch_fits(s, f, t, step_cand)) {
        const unsigned nw = s.bthr / 64;
        rt::FusedLay &lay = s.lay;
        s.kind       = step_cand ? RUN_STEP_ONE_LAUNCH : RUN_IMAGE_ONE_LAUNCH;
        s.tile_links = 4 * (size_t) f.n_tiles; // one link per (tile, part)
        // the last tiles of a work-group in four parts of the frequency range (whole groups of 4 frequencies; not
        // worth it below 32 frequencies)
        lay.split  = t.fused_split == 2 ? 0u : (t.fused_split == 3 ? 2u : 1u);
        lay.k_part = f.K >= 32 && s.emis ? (unsigned) (((f.K + 3) / 4 + 3) / 4 * 4) : 0u;
        // a quarter of the work-group -- its last, youngest waves, one per SIMD -- never marches (rt_fused.hip);
        // gain-only: the same, all of them with a buffer beside the tables (four measured better than five or six)
        lay.n_consumers = knob(t.fused_consumers, s.emis ? nw / 4 : (lay.n_free < nw / 4 ? lay.n_free : nw / 4), nw > 1 ? nw - 1 : 0);
        if (lay.n_consumers >= nw)
            lay.n_consumers = nw - 1;
        lay.consumers_first = t.fused_consumers_first;
        s.chunk = (s.chunk + 32) / 64 * 64; // whole tiles per reservation (64 ... 192 rays)
        s.chunk = s.chunk < 64 ? 64 : s.chunk;
        s.fgrid = one_wg_per_cu(f.n_rays, s.bthr, f.cu_count);
        // (gain-only: the waves that run the frequency pass during the march are the youngest of their SIMD already,
        // nothing starves the last marchers: no late zone)
        if (s.emis)
            late_zone(s, t, f.n_rays, s.fgrid, nw - lay.n_consumers, lay.consumers_first ? lay.n_consumers : 0u, t.late_x10);
        s.fetch_shift = fetch_shift_of((unsigned long long) s.grid * nw);
        return s;
    }
    // (the march as a kernel of its own: the end of the list for the oldest wave of every SIMD as well -- its tail is the
    // drain of the last rays, and one wave per SIMD runs it at the pace of a wave that has the SIMD to itself)
    if (s.n_launch == 1 && s.lds_tab && s.grid > 0)
        late_zone(s, t, f.n_rays, s.grid, s.bthr / 64, 0u, t.late2_x10);
    return s;
}

// ---- the second pass -----------------------------------------------------------------------------------------------
// the records a step run of these facts leaves (rt_records.h): the one place that decides kind and counts
inline RecordSet record_set(const RunFacts &f)
{
    RecordSet r;
    if (!f.step_on || f.path_on || f.spectra_on)
        return r;
    // (use_emis with n_seed > 0: ASE seeds, of the scan where it is on -- no other plan presents that pair)
    // (... and of the suffix scan: rscan() with use_emis and n_seed > 0, the march the plain suffix-scan march)
    // (... or, on a seeded plan, the seeds of the suffix scan: rscan() without use_emis and n_seed > 0, the same march)
    r.kind   = f.rscan() ? (f.n_seed > 0 ? (f.use_emis ? REC_RSCAN_ASE_SEEDS : REC_RSCAN_SEEDS) : REC_RSCAN) : f.scan_on ? (f.n_seed > 0 ? (f.use_emis ? REC_SCAN_ASE_SEEDS : REC_SCAN_SEEDS) : REC_SCAN) : f.n_seed > 0 ? (f.use_emis ? REC_ASE_SEEDS : REC_SEEDS) : REC_NONE;
    r.n_seed = f.n_seed;
    r.L      = f.scan_on ? f.L : 0;
    return r;
}

// the rows a per-ray spectra run of these facts leaves (rt_records.h): the one place that decides kind and counts
inline RowSet row_set(const RunFacts &f)
{
    RowSet r;
    if (f.path_on || (!f.spectra_on && !f.length_spectra_on))
        return r;
    // (n_seed > 0 beside one of the two spectra modes: the seeds of rt_hip_plan_set_spectra_seeds -- a set and the seeds of a
    // scan live in step mode only; the march is that of the single-seed mode, it knows nothing of a seed)
    // (... on an emission plan in spectra mode they are the seeds of rt_hip_plan_set_spectra_ase_seeds: the ASE rows and a block per seed)
    // (... and in length spectra those of rt_hip_plan_set_length_spectra_ase_seeds: the ASE curve and a curve per seed)
    r.kind   = f.spectra_on ? (f.n_seed > 0 ? (f.use_emis ? ROWS_SPEC_ASE_SEEDS : ROWS_SPEC_SEEDS) : ROWS_SPEC)
                            : f.n_seed > 0 ? (f.use_emis ? ROWS_LSPEC_ASE_SEEDS : ROWS_LSPEC_SEEDS) : ROWS_LSPEC;
    r.n_seed = f.n_seed;
    r.L      = r.lengths() ? f.L : 0;
    r.n_rays = (size_t) f.n_rays;
    return r;
}

inline PassKind pass_kind(const RunFacts &f)
{
    if (f.path_on)
        return PASS_PATH;
    // (the passes that leave per-ray spectra, one 16-wave work-group per CU with the staging rows of rt_spec.hip and no histogram:
    // spectra_pass(kind), rt_records.h)
    if (row_set(f).any())
        return row_set(f).pass_kind();
    return f.step_on ? record_set(f).pass_kind() : PASS_FREQ;
}

struct PassShape {
    int wg_waves = 0, nslot = 0;
    bool in_lds  = false; // the I_ang histogram(s) of a work-group in LDS
    size_t lds   = 0;
    unsigned grid = 0, fetch_shift = 0;
};

// the frequency kernel: work-groups of wg_waves waves; the register budget allows `waves` per SIMD, i.e. wg_per_cu work-groups.
// Per-wave row cache for tiles with several pixel runs (seeded): up to 16 rows of Kp doubles, as many as fit
// into the work-group's share of the 160 KB beside the exponent tables, the I_ang histogram and the per-wave
// transposition rows (rt_freq.hip: freq_lds_doubles); fewer than 4 rows is not worth having.
inline void freq_pass_shape(PassShape &s, const RunFacts &f, const Tuning &t)
{
    const bool emis = f.use_emis, excl = f.use_emis && f.exclusive; // (rt_hip_plan_set_ray_grid grants the exclusive mode with emission only)
    const int waves = emis ? rt::FREQ_WAVES : rt::FREQ_WAVES_SEED;
    s.wg_waves      = (int) t.freq_wg_waves;
    int wg_per_cu   = waves * 4 / s.wg_waves;
    wg_per_cu       = wg_per_cu < 1 ? 1 : wg_per_cu;
    auto lds_of     = [&](int rows) { return rt::freq_lds_doubles(s.in_lds, (int) f.n_iang, excl, rows, f.Kp, s.wg_waves) * sizeof(double); };
    auto rows_that_fit = [&](size_t budget) {
        int rows = 0;
        while (rows < 16 && lds_of(rows + 1) + 1024 <= budget)
            rows++;
        return rows;
    };
    if (!excl) { // (exclusive mode: no reduction at all; the space holds the store staging rows instead)
        s.nslot = rows_that_fit(f.lds_limit / (size_t) wg_per_cu);
        if (!emis && s.nslot < (int) t.freq_min_rows && wg_per_cu > 1) { // seeded tiles hold ~7 pixels: rather one work-group less per CU than no row for them
            wg_per_cu--;
            s.nslot = rows_that_fit(f.lds_limit / (size_t) wg_per_cu);
        }
        s.nslot = s.nslot < 4 ? 0 : s.nslot;
    }
    s.lds = lds_of(s.nslot);
    // persistent grid: as many work-groups per CU as LDS (160 KB) and the wave slots allow; the
    // occupancy API under-reports large-LDS kernels, and an over-sized grid is harmless here
    // (surplus work-groups find the tile counter exhausted and leave)
    int per_cu = (int) (f.lds_limit / (s.lds + 512));
    per_cu     = per_cu > wg_per_cu ? wg_per_cu : (per_cu < 1 ? 1 : per_cu);
    per_cu     = (int) knob(t.freq_wgs, (unsigned) per_cu);
    const unsigned long long want = ((unsigned long long) f.n_tiles + (unsigned) s.wg_waves - 1) / (unsigned) s.wg_waves;
    const unsigned long long cap  = (unsigned long long) f.cu_count * (unsigned) per_cu;
    s.grid = (unsigned) (want < cap ? want : cap);
}

// What the second pass of a two-kernel run over all tiles looks like (PASS_PATH: nothing to decide, all zero).
inline PassShape pass_shape(PassKind kind, const RunFacts &f, const Tuning &t)
{
    PassShape s;
    if (kind == PASS_PATH)
        return s;
    // (one global atomic per ray on na*nb addresses serialises badly: the histogram stays in LDS)
    s.in_lds = !spectra_pass(kind) && f.n_iang * sizeof(double) <= 32 * 1024;
    if (kind == PASS_FREQ)
        freq_pass_shape(s, f, t);
    else {
        // spectra, step, step of a seed set, of a length scan or of a scan with its seeds: one 16-wave work-group per CU
        s.wg_waves = rt::FREQ_WG_WAVES;
        // (length spectra: RT_HIP_FREQ_WG_WAVES applies, for the measurement of fewer waves per work-group -- DESIGN.md 4.18,
        // staging candidate (c); the default is the sixteen of every pass here)
        if (kind == PASS_SPEC_SCAN)
            s.wg_waves = (int) t.freq_wg_waves;
        // (a seed set keeps one I_ang histogram and one E_v accumulator per seed, a length scan one of each per length, a scan
        // with scan seeds one of each per (seed, length), an emission plan with ASE seeds one of each for ASE and per seed -- with
        // the scan on, of those per length; a suffix scan one of each per length, with ASE seeds one per (record, length), with
        // scan seeds one per (seed, length))
        const int n_rec      = kind == PASS_STEP || spectra_pass(kind) ? 1 : record_set(f).n_rec();
        const int ang_stride = kind == PASS_STEP ? rt::step_ang_stride((int) f.n_iang) : rt::seeds_ang_stride((int) f.n_iang);
        auto step_lds        = [&](bool in_lds) { return rt::step_lds_doubles(in_lds, ang_stride, f.Kp, s.wg_waves, n_rec) * sizeof(double); };
        // (spectra: the staging rows of 16 waves and the exponent tables take 148 KB of LDS; length spectra cut the same rows
        // into VEC frequencies of four lengths, rt_spec_scan.hip; with the seeds of rt_hip_plan_set_spectra_seeds the seeds share
        // the one staging of a wave, rt_spec_seeds.hip and rt_spec_scan_seeds.hip: the LDS is that of the single-seed pass; so do the
        // two halves of rt_spec_ase_seeds.hip and of rt_spec_scan_ase_seeds.hip, one after the other)
        s.lds = spectra_pass(kind) ? rt::spec_lds_doubles(s.wg_waves) * sizeof(double) : step_lds(s.in_lds);
        if ((kind == PASS_SEEDS || kind == PASS_SCAN || kind == PASS_SCAN_SEEDS || kind == PASS_ASE_SEEDS || kind == PASS_SCAN_ASE_SEEDS ||
             kind == PASS_RSCAN || kind == PASS_RSCAN_ASE_SEEDS || kind == PASS_RSCAN_SEEDS) && s.in_lds &&
            s.lds > f.lds_limit) { // one histogram per record does not fit: global atomics
            s.in_lds = false;
            s.lds    = step_lds(false);
        }
        s.grid = one_wg_per_cu(f.n_tiles, (unsigned) s.wg_waves, f.cu_count);
        if (!spectra_pass(kind) && t.step_serial == 1) { // one wave, one work-group: sums in a fixed order (Tuning::step_serial)
            s.wg_waves = 1;
            s.lds      = step_lds(s.in_lds);
            s.grid     = f.n_tiles ? 1u : 0u;
        }
    }
    s.fetch_shift = fetch_shift_of((unsigned long long) s.grid * (unsigned) s.wg_waves);
    return s;
}

} // namespace rtr
