// rt_runtime.h -- what the host-side translation units of librt_hip.so share (internal, not part of the C ABI).
//
// The C ABI of include/rt_hip.h is implemented by seven translation units:
//   rt_pool.hip     error text, device-memory pool, leased queues, environment overrides
//   rt_plan.hip     the plan: arena packing, ray list / ray grid, run, fetch, probe and path outputs,
//                   rt_hip_image_loop (the host-pointer entry the C++ adapter calls)
//   rt_raygrid.hip  a ray list that is really a tensor grid: recognition + bit-wise verification,
//                   list-mode launch tangents and the probe of the host's libm
//   rt_launch.hip   the kernels (rt_march.hip, rt_freq.hip, rt_path.hip, rt_spec.hip, rt_step.hip, rt_step_seeds.hip, rt_fused_step.hip,
//                   rt_step_scan.hip, rt_step_scan_seeds.hip, rt_step_ase_seeds.hip, rt_spec_scan.hip, rt_spec_seeds.hip, rt_spec_scan_seeds.hip, rt_spec_ase_seeds.hip, rt_spec_scan_ase_seeds.hip; rt_spec_wg.inc the kernel shell the six spectra passes share) and how a run puts them on a queue:
//                   WHAT a run looks like -- tables in LDS or not, one launch or two, instance, grid, chunk, late zone, the
//                   LDS layout of a one-launch run, the shape of the second pass -- is decided by pure functions of plain
//                   numbers (rt_run_shape.h, included by rt_launch.hip alone: RunFacts from the plan + Tuning from the
//                   environment -> run_shape / pass_shape / record_set; rt_hip_debug_run_shape hands them to tests without a
//                   device; which records a step run leaves and how they are numbered is RecordSet, rt_records.h: the plan
//                   keeps the one of its last run, and rt_plan.hip serves the records by it; RowSet is the same for the rows of a
//                   per-ray spectra run);
//                   plan_launch_run enqueues what they say and writes nothing per-launch into the plan's DevParams
//   rt_multi.hip    all devices of the node: RCCL loader, communicator, rt_hip_multi_image_loop, rt_hip_multi_step_loop
//   rt_tables.hip   the gain tables of a resident plan rewritten in place: scan and pack kernels, rt_hip_plan_update_gain
//   rt_history.hip  the step history of a time loop: the records of the last step run filed into slab i of arrays that live in
//                   the plan, by two small launches and no host wait (rt_hip_plan_history_*, rt_hip_debug_history_layout)
// Only rt_launch.hip, rt_multi.hip, rt_tables.hip and rt_history.hip contain device code.
#pragma once

#include "rt_device.h"
#include "rt_records.h"
#include "rt_spec.h"
#include "rt_step.h"

#include <chrono>
#include <cstddef>
#include <string>
#include <vector>

namespace rtr {

// The step history of a plan (rt_history.hip; include/rt_hip.h, rt_hip_plan_history_create): ONE allocation from the pool,
// laid out by history_layout, made and zeroed at the first append and bound to that run's record set and beam sizes.
struct History {
    int n_steps = 0;              // 0: no history
    bool bound  = false;          // the first append has run: dev, lay, recs and n_rec are set
    RecordSet recs;               // ... of that run
    int n_rec = 0;                // its blocks (REC_NONE: the one step record)
    int nv = 0, nx = 0, ny = 0, na = 0, nb = 0;
    unsigned char *dev = nullptr;
    rt_hip_history_layout lay = {};
    std::vector<unsigned char> filled; // host copy of filled[]: which slots an append was queued for
    // behind the last append: whatever zeroes, rewrites or frees a buffer the append reads waits for it (history_wait), a
    // run on another queue waits for it on that queue (rt_hip_plan_run), as tab_ev / tab_pending do for the table pack
    hipEvent_t ev      = nullptr;
    bool pending       = false;
    hipStream_t stream = nullptr; // the queue of the last append
};

} // namespace rtr

// One prepared problem on one device (opaque in include/rt_hip.h).
struct rt_hip_plan {
    int device         = 0;
    int cu_count       = 0;
    rt::DevParams P    = {};
    unsigned char *arena = nullptr;
    size_t arena_bytes = 0;
    void *staging        = nullptr; // page-locked source of an arena upload still in flight on upload_q (plan_create_on)
    hipStream_t upload_q = nullptr;
    unsigned char *out_staging = nullptr; // page-locked copy of the last run's outputs, queued behind its kernels (plan_stage_outputs)
    bool out_staged            = false;
    size_t out_staging_bytes   = 0;
    rt_ray *rays_dev   = nullptr;
    double *grid_dev   = nullptr; // ray grids when rays are generated
    float *tan_dev     = nullptr; // tangents: grid mode [nga + ngb], list mode [2 n_rays]
    double *seedtab_dev = nullptr; // grid mode with a seed: per-axis seed factors + support flags
    std::vector<double> beam_x, beam_y, beam_a, beam_b; // host copies, to recognise ray grid == beam grid
    unsigned char *rec = nullptr; // per-ray march records (two-kernel path)
    bool path_on       = false;   // path tracer instead of the image (rt_hip_plan_enable_path)
    float *path_dev    = nullptr; // [n_rays][3L+1][3]
    int32_t *path_err  = nullptr; // [n_rays]
    size_t path_rays   = 0;
    // spectra mode (rt_hip_plan_enable_spectra): per-ray spectra instead of the image.  Two buffer sets, so that the
    // host-pointer entry (rt_hip_calc_rays) can download one chunk while the next runs; a plan of its own uses set 0.
    bool spectra_on    = false;
    // the rows the last run left (rt_records.h: kind, seeds, lengths and the ray count of THAT run; ROWS_NONE: it was no spectra
    // run, of either mode) -- the accessors of rt_plan.hip serve the rows by it, never by what the plan has been given since
    rtr::RowSet last_rows;
    unsigned spec_sel  = 0;       // buffer set the next run writes
    unsigned spec_last = 0;       // ... and the one the last run wrote
    rt::SpecOut spec[2] = {};
    size_t spec_rays[2] = { 0, 0 }; // rays each set has room for
    // length spectra (rt_hip_plan_enable_length_spectra): what spectra mode leaves, at every length n = 2 .. N from one scan
    // march (rt_spec_scan.hip).  A mode of its own: never together with step, spectra, path, a scan or any seeds.  One
    // allocation from the pool, Iv [L][n][K] | ray2 [L][n] | err [L][n], not zeroed: the kernel writes every element.  The
    // boundary states of the march live in scan_bnd (below) while the mode is on, as a scan's do.
    bool lspec_on      = false;
    bool lspec_first_done = false; // the report of more than RT_N_FAILED_MAX failing rays of the last run with several blocks of rows has been put into list order
    rt::SpecOut lspec  = {};      // block n - 2 of each array: the rows of the sub-problem of n lengths
    unsigned char *lspec_dev = nullptr;
    size_t lspec_bytes = 0;
    // the seeds of the two spectra modes (rt_hip_plan_set_spectra_seeds): 1 .. RT_N_SEED_MAX seed beams whose per-ray outputs
    // one march serves (rt_spec_seeds.hip, rt_spec_scan_seeds.hip).  They travel as a set's do (seed_set, seedset_arena, the
    // factor tables on a forward ray grid) under a count of their own: n_seed and n_scan_seed stay 0 beside them, so every
    // refusal that names a set or the seeds of a scan reads as it did.  Iv and err of a run are seed-major, block 0 seed 0.
    int n_spec_seed    = 0;
    // ... on an EMISSION plan in spectra mode they are the seeds of rt_hip_plan_set_spectra_ase_seeds (rt_spec_ase_seeds.hip):
    // P.use_emis with n_spec_seed > 0 -- no other plan presents that pair.  A run then leaves 1 + n_spec_seed blocks, block 0 the
    // ASE rows.  With length spectra on they are the seeds of rt_hip_plan_set_length_spectra_ase_seeds (rt_spec_scan_ase_seeds.hip): a
    // run leaves (1 + n_spec_seed) (N - 1) blocks, the ASE curve first.
    // step mode (rt_hip_plan_enable_step): E_v and nf instead of the image cube.  One allocation, zeroed by the run's
    // zeroing launch: E_v [K] at its start, nf [nx * ny] behind it at a 256-byte boundary.
    bool step_on       = false;
    bool last_step     = false;   // the last run was a step run
    double *step_dev   = nullptr;
    size_t step_doubles = 0;      // doubles of the allocation
    rt::StepOut step   = {};      // E_v and nf of the last step run (the plan's own or the caller's)
    // the caller's E_v [K] and nf [nx * ny] (rt_hip_plan_set_step_buffers; both NULL: the plan's own allocation above), taken
    // by the next step run; last_step_lent: the last step run wrote the caller's
    double *step_ev_lent = nullptr, *step_nf_lent = nullptr;
    bool last_step_lent  = false;
    // the seeds a step run takes beside the creation seed: up to RT_N_SEED_MAX profiles, installed as a seed set
    // (rt_hip_plan_set_seeds, a seeded plan: n_seed), as the seeds of a length scan (rt_hip_plan_set_scan_seeds, while the scan
    // is on: n_scan_seed, n_seed stays 0) or as ASE seeds (rt_hip_plan_set_ase_seeds, an EMISSION plan: n_seed with
    // P.use_emis, the one case of use_emis with n_seed > 0; ase_scale[s] is the scale of seed s) or as the ASE seeds of a
    // scan (rt_hip_plan_set_scan_ase_seeds, an emission plan while the scan is on: n_scan_seed with P.use_emis; on a backward
    // plan rt_hip_plan_set_suffix_ase_seeds, while the suffix scan is on: the same two fields; on a SEEDED backward plan
    // rt_hip_plan_set_suffix_seeds, while the suffix scan is on: n_scan_seed without P.use_emis).  A set and a scan exclude
    // each other, so their tables live in the same place: one device block (seedset_arena; seed_set[s] points into it, f[4]
    // padded to Kp) and, on a forward ray grid, per seed what seedtab_dev holds for the creation seed (seedset_tab).
    int n_seed      = 0;
    int n_scan_seed = 0;
    rt::DevSeed seed_set[RT_N_SEED_MAX] = {};
    unsigned char *seedset_arena = nullptr;
    unsigned char *seedset_tab   = nullptr;
    const double *seedset_sf[RT_N_SEED_MAX]         = {};
    const unsigned char *seedset_sin[RT_N_SEED_MAX] = {};
    double ase_scale[RT_N_SEED_MAX] = {};
    // length scan (rt_hip_plan_enable_length_scan): one step record per plasma length n = 2 .. N from one forward march;
    // scan_bnd holds the state with which every ray crossed every length boundary (rt_march.hip, scan_bnd_off), from the
    // plan's pool while the scan is on.  On a backward plan (P.method == 1) scan_on is the suffix scan
    // (rt_hip_plan_enable_suffix_scan): one record per run of the LAST n lengths from one backward march, the same boundary
    // buffer and the same records; a plan's method never changes, so the pair says which of the two is on.
    bool scan_on          = false;
    unsigned char *scan_bnd = nullptr;
    size_t scan_bnd_bytes = 0;
    // the records of such a run (rt_records.h says which, and how they are numbered): ONE allocation, zeroed by the run's
    // zeroing launch, of n_rec() blocks of recs_stride doubles, each
    // E_v [K] | pad to 256 bytes | nf [nx * ny] + spare | I_ang [na * nb] + spare (the per-device buffer of rt_multi.hip).
    double *recs_dev    = nullptr;
    size_t recs_doubles = 0;                                  // doubles of the allocation
    size_t recs_stride = 0, recs_nf_off = 0, recs_ang_off = 0; // doubles: block to block, E_v to nf, E_v to I_ang
    rtr::RecordSet last_records;                              // what the last run left there (REC_NONE: nothing, or no step run)
    size_t bad_word = 1; // bytes per ray of bad_dev in the last checking repeat (RecordSet::bad_word)
    size_t rec_bytes   = 0;
    hipEvent_t evm     = nullptr; // between march and frequency kernels
    const rt_ray *host_rays = nullptr; // ray list still on the host, uploaded by the next run (rt_hip_image_loop)
    double *image_own  = nullptr;
    double *iang_own   = nullptr;
    rt::DevCtl *ctl    = nullptr;
    size_t n_image = 0, n_iang = 0;
    unsigned long long n_rays = 0;
    // probe
    bool probe_on        = false;
    unsigned char *probe = nullptr;
    size_t probe_rays    = 0;
    // last run
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t last_stream = nullptr;
    // the queue a run has put work on, set BEFORE its first enqueue: a run that fails midway (a launch error, an
    // allocation) leaves `ran` as it was, and plan_quiesce still has to wait for what was already queued
    hipStream_t queued_stream = nullptr;
    bool queued = false;
    double *last_image = nullptr, *last_iang = nullptr;
    bool ran = false;
    // timing ring (rt_hip_plan_set_timing_ring): event triples of the last runs, so that a caller can time
    // many back-to-back runs without waiting for each; ev0 / evm / ev1 above are the current run's triple
    std::vector<hipEvent_t> ring; // 3 per slot
    unsigned long long runs = 0;
    bool repeated = false; // the checking repeat of the frequency pass has run for the last run
    unsigned char *bad_dev = nullptr; // failing-ray marks of the checking repeat (plan_repeat_checked)
    size_t bad_rays        = 0;
    std::chrono::steady_clock::time_point t_created;
    // frequency kernel arguments that are not part of DevParams (rt_device.h: FreqHot)
    std::vector<const float *> gv_dev; // [N] lineshape table of every length on the device, entry 0 unused
    const double *dv2_dev = nullptr;   // [Kp] 2 * beam.dv
    bool gv_has_nan       = false;     // host scan of the lineshape tables (emission mode): a NaN or an infinity
    // the refractive-index tables and the segment length lie in the ranges under which the march's divisions
    // need no scaling (rt_march.hip, template parameter BOUNDED); checked by rt_hip_plan_create
    bool tables_bounded   = false;
    // the integrator's loop condition |n - n0| < 0.05 (Helper.h:280) holds in every step these tables allow (proved by
    // rt_hip_plan_create from the largest index difference between neighbouring nodes): the march may go without it
    bool ntest_proven     = false;
    // RT_HIP_MARCH_PRUNE (read by rt_hip_plan_create; 0: the march without the step-candidate pruning and with the
    // |n - n0| test, whatever the tables allow) and the instance the last run took (rt_hip_plan_last_march_instance)
    int march_prune       = 1; // (2: h2 / h4 pruned at every launch size)
    int last_march_inst   = 0;
    // links of the fused kernel's work-group tile lists (rt_fused.hip), one word per 64-ray tile; last run fused?
    unsigned *tile_next   = nullptr;
    size_t tile_next_n    = 0;
    bool last_fused       = false;
    // step runs as ONE launch where that applies (rt_fused_step.hip): rt_hip_plan_set_step_one_launch, initial value from
    // RT_HIP_STEP_ONE_LAUNCH at plan creation; off: every step run is the march and rt_step_kernel
    bool step_one_launch  = false;
    // LDS a work-group may ask for on this device (hipDeviceAttributeMaxSharedMemoryPerBlock; 160 KB on gfx950)
    size_t lds_limit      = 0;
    // rt_hip_plan_update_gain (rt_tables.hip).  What rt_hip_plan_create derives from the GRIDS of a length, kept so that
    // an update recomputes tables_bounded and ntest_proven from the scan of the new values alone, and where its nodes lie
    struct TableShape {
        int Nx = 0, Ny = 0;
        double w_min = 0.0;                // smallest grid spacing of both axes
        double fy    = 1.2;                // weight of the edge differences of gyn (mirrored half plane)
        size_t off_node = 0;               // Node[Nx * Ny] of the length: byte offset inside the march blob
    };
    std::vector<TableShape> tab; // [N], entry 0 unused
    bool dz_bounded = false;     // beam.dz lies in the range tables_bounded asks for
    unsigned char *tab_work = nullptr; // device: [descriptors | partials of the scan], grown on demand
    unsigned char *tab_pin  = nullptr; // ... and its page-locked twin
    size_t tab_work_bytes   = 0;
    hipEvent_t tab_ev = nullptr; // behind the pack of the last update: the next run waits for it on its own queue
    bool tab_pending  = false;
    hipEvent_t tab_t[3] = { nullptr, nullptr, nullptr }; // RT_HIP_TIMING: before / behind the scan, before the pack
    rtr::History hist; // the step history (rt_history.hip)
};

namespace rtr {

// ---- rt_pool.hip -------------------------------------------------------------------------------------
// text of the last failure on this thread (rt_hip_last_error)
std::string &last_error();
int fail_hip(hipError_t e, const char *what, const char *file, int line);
int fail_arg(const char *msg);

#define HIP_TRY(expr)                                                \
    do {                                                             \
        hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess)                                        \
            return rtr::fail_hip(e_, #expr, __FILE__, __LINE__);     \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Device-memory pool: allocations (never data) kept across calls, per device.
hipError_t pool_alloc(int device, void **out, size_t bytes);
void pool_free(int device, void *ptr);
void pool_trim_all();
// hipMalloc for the large one-off allocations: out of memory while the pool still parks blocks -> trim and retry
hipError_t dev_malloc(void **out, size_t bytes);
// page-locked host staging for uploads that run beside host work (parked like device blocks; rt_pool.hip)
hipError_t pinned_alloc(void **out, size_t bytes);
void pinned_free(void *ptr);

// tuning overrides from the environment: a missing, non-numeric or non-positive value keeps the default
unsigned env_unsigned(const char *name, unsigned def, unsigned lo, unsigned hi);
// host threads for the list verification and the host tangents (RT_HIP_HOST_THREADS), at most `cap`
unsigned host_threads(unsigned cap);

// non-blocking queues of a device, leased per call and kept across calls
hipStream_t lease_queue(int device);
void release_queue(int device, hipStream_t q);

// ---- rt_plan.hip -------------------------------------------------------------------------------------
// wait for the plan's last run before any of its buffers is freed or parked
void plan_quiesce(rt_hip_plan *p);
// the list stays on the host until the run, which uploads it in slices beside the march
int plan_set_rays_deferred(rt_hip_plan *p, const rt_ray *rays, size_t n_rays);
// after rt_hip_plan_run: queues the download of control block, I_ang and image (step mode: E_v and nf) -- if they are small -- behind the kernels, into
// page-locked staging, so that rt_hip_plan_fetch finds them on the host when the queue has drained
void plan_stage_outputs(rt_hip_plan *p);
// rt_hip_plan_create with the table upload queued on `upload_q` from page-locked staging instead of waited for (nullptr:
// what rt_hip_plan_create does).  Everything that reads the tables must then run on that queue, or after a wait for it.
int plan_create_on(rt_hip_plan **out, hipStream_t upload_q, int device, int N, const rt_beam *beam, const rt_gain *gain,
                   const rt_seed *seed, int method, double scale);
// what rt_hip_plan_fetch does before it copies: wait for the last run, read the control block, repeat a run whose rays
// failed with -2 / -3 in the checking mode (the plan must have run)
int plan_settle_last_run(rt_hip_plan *p);
// the factor tables of every seed of the plan's set on its forward ray grid (rt_seed_tab_kernel), rebuilt whenever the
// grid or the set changes; without a set, a grid or the forward method: none
int plan_build_seedset_tabs(rt_hip_plan *p);
// most rays a list may hold (the kernels index rays with 32 bits)
extern const size_t MAX_LIST_RAYS;
// Where the failure code of a block of a record set lies in the control block, as 32-bit words from its start: word
// base + (block / div) row + block % div.  The ONE place that knows which array of DevCtl a kind's kernel writes: the host
// reads a fetched control block through it (record_code, rt_plan.hip), rt_history_finish_kernel the one on the device.
struct CodeSlot {
    unsigned base = 0, div = 1, row = 0;
    unsigned word(int block) const { return base + ((unsigned) block / div) * row + (unsigned) block % div; }
};
inline CodeSlot record_code_slot(const RecordSet &R)
{
    constexpr unsigned W = sizeof(unsigned);
    const unsigned all   = 1u << 30; // (a kind with one row: block / div is 0)
    switch (R.kind) {
    case REC_SEEDS: return { (unsigned) (offsetof(rt::DevCtl, seed_code) / W), all, 0 };
    case REC_ASE_SEEDS: return { (unsigned) (offsetof(rt::DevCtl, rec_code) / W), all, 0 };
    case REC_SCAN:
    case REC_RSCAN: return { (unsigned) (offsetof(rt::DevCtl, len_code) / W), all, 0 };
    case REC_SCAN_SEEDS:
    case REC_RSCAN_SEEDS: return { (unsigned) (offsetof(rt::DevCtl, seed_len_code) / W), (unsigned) R.L, RT_N_SCAN_MAX };
    case REC_SCAN_ASE_SEEDS:
    case REC_RSCAN_ASE_SEEDS: return { (unsigned) (offsetof(rt::DevCtl, rec_len_code) / W), (unsigned) R.L, RT_N_SCAN_MAX };
    default: return { (unsigned) (offsetof(rt::DevCtl, failure_code) / W), all, 0 }; // (block 0: the run's code)
    }
}

// ---- rt_raygrid.hip ----------------------------------------------------------------------------------
struct GridGuess {
    std::vector<double> g[4]; // x, y, a, b as the doubles of the floats the rays carry
};
inline bool same_bits(float a, float b) { return __builtin_memcmp(&a, &b, sizeof(float)) == 0; }
bool guess_ray_grid(const rt_ray *rays, size_t n, GridGuess &G);
bool verify_ray_grid(const rt_ray *rays, size_t n, const GridGuess &G, unsigned threads);
int plan_set_guessed_grid(rt_hip_plan *p, const GridGuess &G, int64_t first, int64_t count, int64_t stride = 1);
// RayTraceImageCPU.cpp:11-16 on the host: grid point i (as the float a ray carries) falls into deposit cell i
bool grid_points_in_own_cells(const double *g, int n, double d);
// x / d for every x < 2^31 as mulhi(x, mul) >> sh (DevRays::div_mul)
void magic_u31(unsigned d, unsigned &mul, unsigned &sh);
// Helper.h:409-410 on host threads, with the host's tanf
void host_tangents(const rt_ray *rays, size_t n, float *sxy);
// 1: the device restatement of tanf equals this host's tanf; 2: list-mode tangents come from the host
int tan_mode(int device);

// ---- rt_launch.hip -----------------------------------------------------------------------------------
// march -> records -> frequency pass (or the path tracer) on `stream`; records ev0 / evm / ev1 of the plan.  Six steps:
// facts and tuning, run_shape, the buffers (records, path, spectra, tile links), ev0, the first kernel(s) with the slice
// upload, the second pass.  The kernels get a copy of p->P with the numbers of the launch in it; of p->P itself only rec,
// path and path_err are set.
int plan_launch_run(rt_hip_plan *p, hipStream_t stream);
// the records the next run of the plan leaves: record_set (rt_run_shape.h) of the plan's facts
RecordSet plan_record_set(const rt_hip_plan *p);
// ... and the rows, where it is a per-ray spectra run: row_set of the same facts
RowSet plan_row_set(const rt_hip_plan *p);
// a run that reported failing rays: repeat the frequency pass (in step mode: the step kernel) without them (the marks and
// the pass of the repeat, DevParams::safe, go to the launch as arguments; p->P stays as it is)
int plan_repeat_checked(rt_hip_plan *p);
int launch_tan(const rt_ray *rays_dev, unsigned long long n, float *sxy_dev, hipStream_t stream);
int launch_seed_tab(const rt::DevSeed &sd, const rt::DevRays &R, size_t n_points, double *sf, unsigned char *sin);
int launch_selftest(unsigned long long *counts_dev);
// zero up to three device ranges (8-byte multiples; NULL = none) with one launch
int launch_zero3(hipStream_t stream, void *a, size_t a_bytes, void *b, size_t b_bytes, void *c, size_t c_bytes);
// ... and four (a step run into the caller's E_v and nf: E_v, nf, I_ang, control block)
int launch_zero4(hipStream_t stream, void *a, size_t a_bytes, void *b, size_t b_bytes, void *c, size_t c_bytes, void *d, size_t d_bytes);

// ---- rt_history.hip ----------------------------------------------------------------------------------
// wait for the last append of the plan's history, if one is still pending (no history, nothing pending: nothing)
void history_wait(rt_hip_plan *p);
// ... and give the history back to the pool (rt_hip_plan_destroy)
void history_release(rt_hip_plan *p);

} // namespace rtr
