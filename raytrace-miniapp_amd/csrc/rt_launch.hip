// rt_launch.hip -- the kernels of the path and how a run puts them on a queue.
//
// Replaces the launch half of RayTraceImageCudaLoop (src/RayTraceImageCuda.cu:198-203: one thread-per-ray
// launch): a run is the march kernel (persistent lanes over LDS-resident tables, rt_march.hip) -> one
// 96-byte record per ray -> the frequency / deposit kernel (rt_freq.hip), back to back on one queue, or the
// path tracer (rt_path.hip), the spectra kernel (rt_spec.hip) or the step kernel (rt_step.hip) in place of the frequency kernel -- or march and
// frequency / step pass as ONE launch (rt_fused.hip, rt_fused_step.hip).  This is the only translation unit with the
// kernels of the path in it; the rest of the library reaches them through the functions declared in
// rt_runtime.h.  What a run looks like is decided by the pure functions of rt_run_shape.h (facts of the plan + tuning from
// the environment -> RunShape / PassShape); this file selects the instances, fills the argument blocks and enqueues.
#include "rt_path.hip" // debug path tracer (before rt_freq.hip: no FMA contraction there)
#include "rt_freq.hip" // kernel B (includes rt_march.hip, kernel A)
#include "rt_fused.hip" // both as two phases of one launch
#include "rt_spec.hip" // spectra mode: per-ray spectra in place of the deposit
#include "rt_step.hip" // step mode: E_v, nf and I_ang, the image cube reduced on the way
#include "rt_step_seeds.hip" // step mode with a seed set: one record per seed from one march
#include "rt_fused_step.hip" // step mode as two phases of one launch (opt-in)
#include "rt_step_scan.hip" // step mode with a length scan: one record per plasma length from one forward march
#include "rt_step_rscan.hip" // step mode with a suffix scan: one record per run of the last n lengths from one backward march
#include "rt_step_scan_seeds.hip" // ... with the seeds of the scan: one record per (seed, length) from that march
#include "rt_step_ase_seeds.hip"  // step kernel of an emission plan with ASE seeds: the ASE record and one per seed from one march
#include "rt_step_scan_ase_seeds.hip" // ... with the length scan on: that whole record at every length from one forward march
#include "rt_step_rscan_ase_seeds.hip" // ... with the suffix scan on: that whole record of the last n lengths from one backward march

#include "rt_step_rscan_seeds.hip" // the suffix scan of a seeded plan with the seeds of the scan: one record per (seed, run of the last n)
#include "rt_spec_scan.hip" // length spectra: per-ray spectra, exit rays and codes at every length from one scan march
#include "rt_spec_seeds.hip" // spectra mode with the seeds of rt_hip_plan_set_spectra_seeds: those outputs once per seed beam
#include "rt_spec_scan_seeds.hip" // ... and length spectra with them: once per (seed beam, length)
#include "rt_spec_ase_seeds.hip" // spectra mode of an emission plan with the seeds of rt_hip_plan_set_spectra_ase_seeds: the ASE rows and a block per seed beam
#include "rt_spec_scan_ase_seeds.hip" // ... and length spectra of one with the seeds of rt_hip_plan_set_length_spectra_ase_seeds: a block per (curve, length)
// (rt_spec_wg.inc: the kernel shell the six spectra passes above share, as text; rt_spec_tile.inc and rt_spec_scan_tile.inc: their tile text)

#include "rt_runtime.h"
#include "rt_run_shape.h" // what a run looks like: the pure decision (facts + tuning -> shape) this file enqueues

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

using namespace rtr;

namespace {

// Dynamic LDS above 64 KB has to be allowed per kernel and per device; asked for once per (device, kernel), and
// again only when a launch needs more than the attribute stands at.
int allow_lds(const void *kernel, int device, size_t bytes, size_t limit)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> allowed; // the size the attribute stands at
    if (bytes <= 64 * 1024)
        return RT_OK;
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = allowed[{ device, kernel }];
    if (bytes <= have)
        return RT_OK;
    const size_t want = limit > bytes ? limit : bytes;
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) want));
    have = want;
    return RT_OK;
}

// every launch of the path: the LDS attribute where the launch needs it, the launch, its error
template <typename Arg>
int launch(const rt_hip_plan *p, void (*kernel)(const Arg), unsigned grid, unsigned block, size_t lds, hipStream_t stream, const Arg &a)
{
    const int rc = allow_lds(reinterpret_cast<const void *>(kernel), p->device, lds, p->lds_limit);
    if (rc != RT_OK)
        return rc;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, a);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- from a small key to the kernel instance, one function per family ----------------------------------------------
// (the set of instances is what these functions name and nothing else: unbounded tables have no OPT and, of the MODEs,
// only 0 and 1; the global-table march has MODE 0 only; the gain-only one-launch kernel MAXQ = 3 only; the scan instance
// of the march, MODE 3 with MARCH_OPT_SCAN alone, exists for all four combinations of LDS_TAB and BOUNDED, and so do the
// scan instances of the backward march, MODE 1 and MODE 0 with MARCH_OPT_SCAN alone)
using march_fn      = void (*)(const rt::DevParams);
using fused_fn      = void (*)(const rt::FusedKArg);
using fused_step_fn = void (*)(const rt::FusedStepKArg);

// the BOUNDED instances of the march by OPT (rt_march.hip): 0 as before; 3 = h1 pruned, no |n - n0| test; 7 = h2 and h4
// pruned as well
template <bool LDS_TAB, int MODE> march_fn march_bounded(int opt)
{
    return opt == 7 ? rt::rt_march_kernel<LDS_TAB, true, MODE, 7> : opt == 3 ? rt::rt_march_kernel<LDS_TAB, true, MODE, 3> : rt::rt_march_kernel<LDS_TAB, true, MODE, 0>;
}
// the scan instances of the backward march (the suffix scan, rt_step_rscan.hip): MODE 1 for an emission plan, MODE 0 for a
// seeded one, the four combinations of LDS_TAB and BOUNDED each
template <int MODE> march_fn march_rscan(bool lds_tab, bool bounded)
{
    return lds_tab ? (bounded ? rt::rt_march_kernel<true, true, MODE, rt::MARCH_OPT_SCAN> : rt::rt_march_kernel<true, false, MODE, rt::MARCH_OPT_SCAN>)
                   : (bounded ? rt::rt_march_kernel<false, true, MODE, rt::MARCH_OPT_SCAN> : rt::rt_march_kernel<false, false, MODE, rt::MARCH_OPT_SCAN>);
}
march_fn march_kernel(bool lds_tab, bool bounded, int mode, int opt)
{
    if ((opt & rt::MARCH_OPT_SCAN) && mode != 3) // the suffix scan: the backward march with the boundary stores, no pruning
        return mode == 1 ? march_rscan<1>(lds_tab, bounded) : march_rscan<0>(lds_tab, bounded);
    if (opt & rt::MARCH_OPT_SCAN) // the length scan: forward method at compile time (MODE 3), boundary stores, no pruning
        return lds_tab ? (bounded ? rt::rt_march_kernel<true, true, 3, rt::MARCH_OPT_SCAN> : rt::rt_march_kernel<true, false, 3, rt::MARCH_OPT_SCAN>)
                       : (bounded ? rt::rt_march_kernel<false, true, 3, rt::MARCH_OPT_SCAN> : rt::rt_march_kernel<false, false, 3, rt::MARCH_OPT_SCAN>);
    if (!lds_tab)
        return bounded ? march_bounded<false, 0>(opt) : rt::rt_march_kernel<false, false, 0>;
    if (!bounded)
        return mode == 1 ? rt::rt_march_kernel<true, false, 1> : rt::rt_march_kernel<true, false, 0>;
    return mode == 1 ? march_bounded<true, 1>(opt) : mode == 2 ? march_bounded<true, 2>(opt) : mode == 3 ? march_bounded<true, 3>(opt)
         : mode == 4 ? march_bounded<true, 4>(opt) : march_bounded<true, 0>(opt);
}

template <int SF, int MAXQ, bool EMIS> fused_fn fused_bounded(int opt)
{
    return opt == 7 ? rt::rt_fused_kernel<true, SF, MAXQ, EMIS, 7> : opt == 3 ? rt::rt_fused_kernel<true, SF, MAXQ, EMIS, 3> : rt::rt_fused_kernel<true, SF, MAXQ, EMIS, 0>;
}
template <int SF> fused_fn fused_kernel_sf(bool bounded, int maxq, bool emis, int opt)
{
    if (!emis)
        return bounded ? fused_bounded<SF, 3, false>(opt) : rt::rt_fused_kernel<false, SF, 3, false>;
    if (maxq == 2)
        return bounded ? fused_bounded<SF, 2, true>(opt) : rt::rt_fused_kernel<false, SF, 2>;
    return bounded ? fused_bounded<SF, 3, true>(opt) : rt::rt_fused_kernel<false, SF, 3>;
}
fused_fn fused_kernel(bool bounded, bool s6, int maxq, bool emis, int opt)
{
    return s6 ? fused_kernel_sf<6>(bounded, maxq, emis, opt) : fused_kernel_sf<0>(bounded, maxq, emis, opt);
}

template <int SF> fused_step_fn fused_step_bounded(int opt)
{
    return opt == 7 ? rt::rt_fused_step_kernel<true, SF, 7> : opt == 3 ? rt::rt_fused_step_kernel<true, SF, 3> : rt::rt_fused_step_kernel<true, SF, 0>;
}
fused_step_fn fused_step_kernel(bool bounded, bool s6, int opt)
{
    return s6 ? (bounded ? fused_step_bounded<6>(opt) : rt::rt_fused_step_kernel<false, 6>)
              : (bounded ? fused_step_bounded<0>(opt) : rt::rt_fused_step_kernel<false, 0>);
}

// frequency kernel variants: SF = compile-time number of sub-segments (6 <=> N = 3, the shipped inputs; 0 = any N)
void (*freq_kernel(bool s6, bool emis, bool excl))(const rt::FreqKArg)
{
    if (emis && excl)
        return s6 ? rt::rt_freq_kernel<6, true, true> : rt::rt_freq_kernel<0, true, true>;
    if (emis)
        return s6 ? rt::rt_freq_kernel<6, true, false> : rt::rt_freq_kernel<0, true, false>;
    return s6 ? rt::rt_freq_kernel<6, false, false> : rt::rt_freq_kernel<0, false, false>;
}
void (*spec_kernel(bool s6, bool emis))(const rt::SpecKArg)
{
    return emis ? (s6 ? rt::rt_spec_kernel<6, true> : rt::rt_spec_kernel<0, true>) : (s6 ? rt::rt_spec_kernel<6, false> : rt::rt_spec_kernel<0, false>);
}
void (*step_kernel(bool s6, bool emis))(const rt::StepKArg)
{
    return emis ? (s6 ? rt::rt_step_kernel<6, true> : rt::rt_step_kernel<0, true>) : (s6 ? rt::rt_step_kernel<6, false> : rt::rt_step_kernel<0, false>);
}
void (*seeds_kernel(bool s6))(const rt::SeedsKArg) { return s6 ? rt::rt_step_seeds_kernel<6> : rt::rt_step_seeds_kernel<0>; }
void (*ase_seeds_kernel(bool s6))(const rt::AseSeedsKArg) { return s6 ? rt::rt_step_ase_seeds_kernel<6> : rt::rt_step_ase_seeds_kernel<0>; }
void (*scan_kernel(bool emis))(const rt::ScanKArg) { return emis ? rt::rt_step_scan_kernel<true> : rt::rt_step_scan_kernel<false>; }
void (*rscan_kernel(bool emis))(const rt::ScanKArg) { return emis ? rt::rt_step_rscan_kernel<true> : rt::rt_step_rscan_kernel<false>; }
void (*spec_scan_kernel(bool emis, bool backward))(const rt::SpecScanKArg)
{
    return emis ? (backward ? rt::rt_spec_scan_kernel<true, true> : rt::rt_spec_scan_kernel<true, false>)
                : (backward ? rt::rt_spec_scan_kernel<false, true> : rt::rt_spec_scan_kernel<false, false>);
}
void (*spec_seeds_kernel(bool s6))(const rt::SpecSeedsKArg) { return s6 ? rt::rt_spec_seeds_kernel<6> : rt::rt_spec_seeds_kernel<0>; }
void (*spec_ase_seeds_kernel(bool s6))(const rt::SpecSeedsKArg) { return s6 ? rt::rt_spec_ase_seeds_kernel<6> : rt::rt_spec_ase_seeds_kernel<0>; }
void (*spec_scan_seeds_kernel(bool backward))(const rt::SpecScanSeedsKArg)
{
    return backward ? rt::rt_spec_scan_seeds_kernel<true> : rt::rt_spec_scan_seeds_kernel<false>;
}
void (*spec_scan_ase_seeds_kernel(bool backward))(const rt::SpecScanSeedsKArg)
{
    return backward ? rt::rt_spec_scan_ase_seeds_kernel<true> : rt::rt_spec_scan_ase_seeds_kernel<false>;
}

// what a launch of the frequency pass covers: tiles [tile_begin, tile_end) on tile counter freq_id (a run is one launch
// over all tiles; the range exists for experiments that split it), and the marks of the checking repeat (DevParams::safe)
struct PassRun {
    unsigned tile_begin, tile_end, freq_id;
    unsigned safe;
    unsigned char *bad;
};

// the frequency pass's own argument block (rt_device.h): hot = what the frequency loop reads, cold = what the
// per-ray preamble of a tile reads
rt::FreqKArg freq_args(const rt_hip_plan *p, bool iang_in_lds, int nslot, unsigned fetch_shift, const PassRun &r)
{
    const rt::DevParams &P = p->P;
    rt::FreqKArg a;
    memset(&a, 0, sizeof(a));
    a.hot.gv0        = p->gv_dev.size() > 1 ? p->gv_dev[1] : nullptr;
    a.hot.gv1        = p->gv_dev.size() > 2 ? p->gv_dev[2] : nullptr;
    a.hot.gain       = P.gain;
    a.hot.rec        = P.rec;
    a.hot.image      = P.image;
    a.hot.iang       = P.iang;
    a.hot.ctl        = P.ctl;
    a.hot.dv2        = p->dv2_dev;
    // (gain-only without a seed -- tables without E0 -- multiplies this row by f0 = 0, as the CPU starts from Iv = 0 and keeps
    // 0 * exp(gl): any finite row of Kp doubles serves, a NULL one is read all the same)
    a.hot.seed_fk    = P.has_seed ? P.seed.f[4] : p->dv2_dev;
    a.hot.bad        = r.bad;
    a.hot.scale      = P.scale;
    a.hot.gs_cap     = P.gs_cap;
    a.hot.K          = P.K;
    a.hot.Kp         = P.Kp;
    a.hot.L          = P.L;
    a.hot.method     = P.method;
    a.hot.rec_stride = P.rec_stride;
    a.hot.n_rays     = (unsigned) P.rays.count;
    a.hot.tile_begin = r.tile_begin;
    a.hot.tile_end   = r.tile_end;
    a.hot.freq_id    = r.freq_id;
    a.hot.fetch_shift = fetch_shift;
    a.hot.nslot      = nslot;
    a.hot.nx         = P.beam.nx;
    a.hot.ny         = P.beam.ny;
    a.hot.n_ang      = P.beam.na * P.beam.nb;
    a.hot.flags      = (P.exclusive ? rt::FQ_EXCLUSIVE : 0u) | (r.safe == 1 ? rt::FQ_SAFE_CHECK : 0u) |
                  (r.safe == 2 ? rt::FQ_SAFE_SKIP : 0u) | (P.exact_emis ? rt::FQ_EXACT_EMIS : 0u) |
                  (P.has_seed ? rt::FQ_HAS_SEED : 0u) | (P.probe_on ? rt::FQ_PROBE : 0u) |
                  (p->gv_has_nan ? rt::FQ_GV_NAN : 0u) | (iang_in_lds ? rt::FQ_IANG_LDS : 0u) |
                  ((P.method != 1 || P.has_seed || P.probe_on) ? rt::FQ_NEED_EXIT : 0u) |
                  (P.own_cells ? rt::FQ_OWN_CELLS : 0u) | ((P.debug & 4u) ? rt::FQ_DBG_NOFLUSH : 0u);
    a.cold.beam  = P.beam;
    a.cold.seed  = P.seed;
    a.cold.rays  = P.rays;
    a.cold.probe = P.probe;
    return a;
}

RunFacts run_facts(const rt_hip_plan *p)
{
    const rt::DevParams &P = p->P;
    RunFacts f;
    f.cu_count        = p->cu_count;
    f.lds_limit       = p->lds_limit;
    f.n_rays          = p->n_rays;
    f.n_tiles         = P.n_tiles;
    f.blob_bytes      = P.blob_bytes;
    f.K               = P.K;
    f.Kp              = P.Kp;
    f.L               = P.L;
    f.n_iang          = p->n_iang;
    f.rays_per_pixel  = P.rays.nga * P.rays.ngb;
    f.n_seed          = p->scan_on ? p->n_scan_seed : p->n_seed; // (a set and the seeds of a scan exclude each other)
    if (p->n_spec_seed > 0) // (the seeds of the two spectra modes: neither a set nor the seeds of a scan is installed beside them)
        f.n_seed = p->n_spec_seed;
    f.c_h3            = P.c_h3;
    f.march_prune     = p->march_prune;
    f.method          = P.method;
    f.safe            = P.safe;
    f.debug           = P.debug;
    f.use_emis        = P.use_emis != 0;
    f.own_cells       = P.own_cells != 0;
    f.exclusive       = P.exclusive != 0;
    f.path_on         = p->path_on;
    f.spectra_on      = p->spectra_on;
    f.step_on         = p->step_on;
    f.step_one_launch = p->step_one_launch;
    f.probe_on        = p->probe_on;
    f.has_ray_list    = P.rays.list != nullptr;
    f.host_rays       = p->host_rays != nullptr;
    f.tables_bounded  = p->tables_bounded;
    f.ntest_proven    = p->ntest_proven;
    f.gv_has_nan      = p->gv_has_nan;
    f.scan_on         = p->scan_on && p->step_on;
    f.length_spectra_on = p->lspec_on;
    return f;
}

// the argument block of a pass that stands in the frequency kernel's place: its two halves, without the cube (never touched)
template <typename KArg> KArg pass_args(const rt::FreqKArg &fa)
{
    KArg a;
    memset(&a, 0, sizeof(a));
    a.hot       = fa.hot;
    a.hot.image = nullptr;
    a.cold      = fa.cold;
    return a;
}

// ---- what the passes with several records share (rt_records.h: the blocks of the plan's one allocation) --------------
// block r as the kernels of a seed set and of ASE seeds take it
rt::SeedRec seed_rec(const rt_hip_plan *p, int r)
{
    double *blk = p->recs_dev + (size_t) r * p->recs_stride;
    return rt::SeedRec{ blk, blk + p->recs_nf_off, blk + p->recs_ang_off };
}
// ... and all of them as the kernels of a length scan do, with the boundary states of the march
void fill_scan(rt::ScanArg &a, const rt_hip_plan *p) { a = rt::ScanArg{ p->scan_bnd, p->recs_dev, p->recs_stride, p->recs_nf_off, p->recs_ang_off }; }
// the tables of the plan's first n_seed seeds; grid_tabs: with their factor tables on the forward ray grid, which must then
// have been built (`who`: the kernel and what it calls them, for the message)
int fill_seed_tabs(rt::SeedTabs &tb, const rt_hip_plan *p, int n_seed, bool grid_tabs, const char *who)
{
    for (int i = 0; i < n_seed; i++) {
        tb.fk[i]   = p->seed_set[i].f[4];
        tb.sf[i]   = grid_tabs ? p->seedset_sf[i] : nullptr;
        tb.sin[i]  = grid_tabs ? p->seedset_sin[i] : nullptr;
        tb.seed[i] = p->seed_set[i];
        if (grid_tabs && (!tb.sf[i] || !tb.sin[i]))
            return fail_arg((std::string(who) + " were not built for this ray grid").c_str());
    }
    return RT_OK;
}

// Whether the seeds' factor tables on the forward ray grid serve this run.  A seeded plan has P.rays.sf exactly then.  An
// emission plan has no creation seed and hence none: there the tables serve a forward ray GRID only, and the ray set
// decides -- a list set behind the grid (rt_hip_plan_set_rays resets P.rays, not the tables) takes seed_factor at its launch
// rays, and a backward run takes it at the state that serves a record, never at a grid point.
bool seeds_on_grid(const rt_hip_plan *p, const RecordKindRow &k)
{
    return k.ase ? p->P.rays.gx && !p->P.rays.list && p->P.method != 1 && p->seedset_sf[0] != nullptr : p->P.rays.sf != nullptr;
}
// What no valid plan reaches: a pass of several records whose buffers or facts are not its kind's.
int records_ready(const rt_hip_plan *p, const RunFacts &f, const RecordSet &R)
{
    const RecordKindRow &k = R.row();
    auto fail = [&](const char *what) { return fail_arg((std::string("step kernel of ") + k.name + what).c_str()); };
    if (!p->recs_dev || (k.lengths && !p->scan_bnd))
        return fail(": the records or the boundary states of this run were not allocated");
    if (p->recs_doubles < (size_t) R.n_rec() * p->recs_stride)
        return fail(": the records of this run are smaller than the blocks of its kind");
    if (k.lengths && f.L > RT_N_SCAN_MAX)
        return fail(": more than RT_N_SCAN_MAX lengths");
    if (k.seeds && (f.n_seed < 1 || f.n_seed > RT_N_SEED_MAX || f.use_emis != k.ase || (k.suffix && f.method != 1)))
        return fail(": not 1 .. RT_N_SEED_MAX seeds on the plan (emission or gain-only, forward or backward) the kind takes");
    return RT_OK;
}
// The argument block of such a pass.  With lengths every record's I_ang lies in its block; the creation seed is not among
// the seeds a kind carries (an emission plan has none); with an ASE record or the suffix form nf of every record goes by
// atomics (the plain store is rt_step_kernel's and the forward kernels' without ASE alone).
template <typename KArg> KArg records_args(const rt::FreqKArg &fa, const RecordKindRow &k)
{
    KArg a = pass_args<KArg>(fa);
    if (k.lengths)
        a.hot.iang = nullptr;
    if (k.seeds)
        a.hot.seed_fk = nullptr;
    if (k.ase || k.suffix)
        a.hot.flags &= ~(unsigned) rt::FQ_EXCLUSIVE;
    return a;
}
// ... its seeds: their count and tables
template <typename Set> int fill_set(Set &set, const rt_hip_plan *p, int n_seed, const RecordKindRow &k)
{
    set.n_seed = n_seed;
    return fill_seed_tabs(set.tabs, p, n_seed, seeds_on_grid(p, k), (std::string("step kernel of ") + k.name + ": the factor tables of the seeds").c_str());
}
// ... the scale of every record: the plan's for the ASE record, its own for a seed's
template <typename Set> void fill_scales(Set &set, const rt_hip_plan *p, int n_seed)
{
    for (int r = 0; r <= n_seed; r++)
        set.scale[r] = r == 0 ? p->P.scale : p->ase_scale[r - 1];
}
// ... and the blocks, for the kernels without lengths (the others take all of them through fill_scan)
template <typename Set> void fill_out(Set &set, const rt_hip_plan *p, int n_rec)
{
    for (int r = 0; r < n_rec; r++)
        set.out[r] = seed_rec(p, r);
}

// The second pass over all tiles as a kernel of its own: the frequency / deposit kernel, or in its place the spectra
// kernel (per-ray spectra, no image), the step kernel (E_v, nf and I_ang, no image cube) or one of the step kernels that
// leave several records (record_set(f) says which kind and how many; the row of the kind, rt_records.h, what its block takes).
int launch_pass(rt_hip_plan *p, const RunFacts &f, const Tuning &t, PassKind kind, hipStream_t stream, unsigned safe = 0, unsigned char *bad = nullptr)
{
    const PassShape s      = pass_shape(kind, f, t);
    const RecordSet R      = record_set(f);
    const RecordKindRow &k = R.row();
    const RowSet W         = row_set(f); // (the rows of a per-ray spectra pass, rt_records.h)
    // (what of a one-work-group-per-CU pass does not fit, by kind; the frequency kernel's message, below, carries figures)
    if (s.lds > f.lds_limit && spectra_pass(kind))
        return fail_arg((std::string(W.row().mode) + ": the staging rows do not fit into the LDS of this device").c_str());
    if (s.lds > f.lds_limit && kind == PASS_STEP)
        return fail_arg("step kernel: the E_v accumulator (nv doubles) does not fit into the LDS of this device");
    if (s.lds > f.lds_limit && kind != PASS_FREQ && kind != PASS_PATH)
        return fail_arg((std::string("step kernel of ") + k.name + ": the E_v accumulators (nv doubles " + k.acc + ") do not fit into the LDS of this device").c_str());
    if (s.grid == 0)
        return RT_OK;
    if (s.lds > f.lds_limit) {
        char msg[256];
        snprintf(msg, sizeof(msg), "frequency kernel: %zu bytes of LDS per work-group (I_ang histogram of %zu cells, %d waves) "
                 "exceed the device's %zu", s.lds, f.n_iang, s.wg_waves, f.lds_limit);
        return fail_arg(msg);
    }
    const rt::FreqKArg fa = freq_args(p, s.in_lds, s.nslot, s.fetch_shift, PassRun{ 0, f.n_tiles, 0, safe, bad });
    const unsigned block  = (unsigned) s.wg_waves * 64;
    if (kind == PASS_FREQ)
        return launch(p, freq_kernel(f.s6(), f.use_emis, f.use_emis && f.exclusive), s.grid, block, s.lds, stream, fa);
    if (spectra_pass(kind)) { // ---- the passes that leave per-ray rows: per kind its argument block and its kernel ----
        const char *who = W.row().who;
        auto fail       = [&](const char *what) { return fail_arg((std::string(who) + what).c_str()); };
        // (the seeds of rt_hip_plan_set_spectra_seeds on a plan created with a seed, of rt_hip_plan_set_spectra_ase_seeds on an emission plan)
        if (W.row().seeds && (f.n_seed < 1 || f.n_seed > RT_N_SEED_MAX || f.use_emis != W.row().ase || (p->P.has_seed != 0) == W.row().ase))
            return fail(W.row().ase ? ": not 1 .. RT_N_SEED_MAX seeds on an emission plan" : ": not 1 .. RT_N_SEED_MAX seeds on a plan created with a seed");
        const rt::SpecOut &out = W.lengths() ? p->lspec : p->spec[p->spec_sel];
        if (kind != PASS_SPEC && (!out.Iv || (W.lengths() && !p->scan_bnd)))
            return fail(W.lengths() ? ": the outputs or the boundary states of this run were not allocated" : ": the outputs of this run were not allocated");
        if (W.lengths() && (f.L < 2 || f.L > RT_N_SCAN_MAX))
            return fail(": not 2 .. RT_N_SCAN_MAX lengths");
        rt::FreqKArg fs = fa;
        fs.hot.iang     = nullptr;
        // (an emission plan has no creation seed and hence no P.rays.sf: the seeds' factor tables serve a forward ray GRID
        // only, and the ray set decides -- seeds_on_grid says the same of the step passes with ASE seeds)
        const bool grid_tabs       = W.row().ase ? p->P.rays.gx && !p->P.rays.list && p->P.method != 1 && p->seedset_sf[0] != nullptr : p->P.rays.sf != nullptr;
        const std::string tabs_who = std::string(who) + ": the factor tables of the seeds";
        if (kind == PASS_SPEC) {
            rt::SpecKArg a = pass_args<rt::SpecKArg>(fs);
            a.out          = out;
            return launch(p, spec_kernel(f.s6(), f.use_emis), s.grid, block, s.lds, stream, a);
        }
        if (kind == PASS_SPEC_SCAN) { // length spectra: the rows of every length, from the boundary states of the scan march
            rt::SpecScanKArg a = pass_args<rt::SpecScanKArg>(fs);
            a.scan             = rt::SpecScanArg{ out, p->scan_bnd };
            return launch(p, spec_scan_kernel(f.use_emis, f.method == 1), s.grid, block, s.lds, stream, a);
        }
        // ... with the seeds of rt_hip_plan_set_spectra_seeds: once per (seed beam, length) -- or, on an emission plan with those of
        // rt_hip_plan_set_length_spectra_ase_seeds, blocks (0, n) the ASE curve and blocks (1 + s, n) the curve of seed s
        if (kind == PASS_SPEC_SCAN_SEEDS || kind == PASS_SPEC_SCAN_ASE_SEEDS) {
            rt::SpecScanSeedsKArg a = pass_args<rt::SpecScanSeedsKArg>(fs);
            if (!W.row().ase) // (the emission half names the row of a plan without a seed, freq_args: never read)
                a.hot.seed_fk = nullptr;
            a.set.n_seed  = f.n_seed;
            a.set.out     = out;
            a.set.bnd     = p->scan_bnd;
            const int rc  = fill_seed_tabs(a.set.tabs, p, f.n_seed, grid_tabs, tabs_who.c_str());
            return rc != RT_OK ? rc : launch(p, W.row().ase ? spec_scan_ase_seeds_kernel(f.method == 1) : spec_scan_seeds_kernel(f.method == 1), s.grid, block, s.lds, stream, a);
        }
        // spectra mode with seeds: once per seed beam -- or, on an emission plan, block 0 ASE and block 1 + s seed s
        rt::SpecSeedsKArg a = pass_args<rt::SpecSeedsKArg>(fs);
        if (!W.row().ase)
            a.hot.seed_fk = nullptr;
        a.set.n_seed = f.n_seed;
        a.set.out    = out;
        const int rc = fill_seed_tabs(a.set.tabs, p, f.n_seed, grid_tabs, tabs_who.c_str());
        return rc != RT_OK ? rc : launch(p, W.row().ase ? spec_ase_seeds_kernel(f.s6()) : spec_seeds_kernel(f.s6()), s.grid, block, s.lds, stream, a);
    }
    if (kind == PASS_STEP) {
        rt::StepKArg a = pass_args<rt::StepKArg>(fa);
        a.out       = p->step;
        return launch(p, step_kernel(f.s6(), f.use_emis), s.grid, block, s.lds, stream, a);
    }
    // ---- the passes that leave several records: per kind its argument block and its kernel ----
    int rc = records_ready(p, f, R);
    if (rc != RT_OK)
        return rc;
    if (kind == PASS_SCAN || kind == PASS_RSCAN) { // one record per length, or per run of the last n lengths (a backward plan)
        rt::ScanKArg a = records_args<rt::ScanKArg>(fa, k);
        fill_scan(a.scan, p);
        return launch(p, k.suffix ? rscan_kernel(f.use_emis) : scan_kernel(f.use_emis), s.grid, block, s.lds, stream, a);
    }
    if (kind == PASS_SCAN_ASE_SEEDS || kind == PASS_RSCAN_ASE_SEEDS) { // an emission plan: one record per (ASE | seed, n)
        rt::ScanAseSeedsKArg a = records_args<rt::ScanAseSeedsKArg>(fa, k);
        fill_scan(a.scan, p);
        fill_scales(a.set, p, f.n_seed);
        rc = fill_set(a.set, p, f.n_seed, k);
        return rc != RT_OK ? rc : launch(p, k.suffix ? rt::rt_step_rscan_ase_seeds_kernel : rt::rt_step_scan_ase_seeds_kernel, s.grid, block, s.lds, stream, a);
    }
    if (kind == PASS_SCAN_SEEDS || kind == PASS_RSCAN_SEEDS) { // a seeded plan (gain-only): one record per (seed, length), or per (seed, run of the last n)
        rt::ScanSeedsKArg a = records_args<rt::ScanSeedsKArg>(fa, k);
        fill_scan(a.scan, p);
        rc = fill_set(a.set, p, f.n_seed, k);
        return rc != RT_OK ? rc : launch(p, k.suffix ? rt::rt_step_rscan_seeds_kernel : rt::rt_step_scan_seeds_kernel, s.grid, block, s.lds, stream, a);
    }
    if (kind == PASS_ASE_SEEDS) { // an emission plan: block 0 the ASE record, block 1 + s the record of seed s
        rt::AseSeedsKArg a = records_args<rt::AseSeedsKArg>(fa, k);
        fill_out(a.set, p, R.n_rec());
        fill_scales(a.set, p, f.n_seed);
        rc = fill_set(a.set, p, f.n_seed, k);
        return rc != RT_OK ? rc : launch(p, ase_seeds_kernel(f.s6()), s.grid, block, s.lds, stream, a);
    }
    // a seed set (a seeded plan: gain-only): one record per seed
    rt::SeedsKArg a = records_args<rt::SeedsKArg>(fa, k);
    fill_out(a.set, p, R.n_rec());
    rc = fill_set(a.set, p, f.n_seed, k);
    return rc != RT_OK ? rc : launch(p, seeds_kernel(f.s6()), s.grid, block, s.lds, stream, a);
}

} // namespace

namespace rt {
// the outputs and the control block of a run zeroed by ONE launch (three hipMemsetAsync are three launches with a
// dependency gap behind each: ~1.5 us apiece, MI355X_MICROARCH.md "boundary" -- a percent of an 8-rank step)
extern "C" __global__ void __launch_bounds__(256) rt_zero_kernel(unsigned long long *a, unsigned long long na, unsigned long long *b,
                                                                unsigned long long nb, unsigned long long *c, unsigned long long nc)
{
    const unsigned long long step = (unsigned long long) gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x; i < na + nb + nc; i += step) {
        unsigned long long *q = i < na ? a + i : (i < na + nb ? b + (i - na) : c + (i - na - nb));
        *q                    = 0ull;
    }
}
// (four ranges: a step run into buffers the caller lent -- E_v, nf, I_ang, control block.  A kernel of its own, so that
// the zeroing launch of every other run stays the instance it was.)
extern "C" __global__ void __launch_bounds__(256) rt_zero4_kernel(unsigned long long *a, unsigned long long na, unsigned long long *b,
                                                                 unsigned long long nb, unsigned long long *c, unsigned long long nc,
                                                                 unsigned long long *d, unsigned long long nd)
{
    const unsigned long long step = (unsigned long long) gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x; i < na + nb + nc + nd; i += step) {
        unsigned long long *q = i < na ? a + i : (i < na + nb ? b + (i - na) : (i < na + nb + nc ? c + (i - na - nb) : d + (i - na - nb - nc)));
        *q                    = 0ull;
    }
}
} // namespace rt

namespace rtr {

int launch_zero4(hipStream_t stream, void *a, size_t a_bytes, void *b, size_t b_bytes, void *c, size_t c_bytes, void *d, size_t d_bytes)
{
    const unsigned long long na = a ? a_bytes / 8 : 0, nb = b ? b_bytes / 8 : 0, nc = c ? c_bytes / 8 : 0, nd = d ? d_bytes / 8 : 0;
    if (na + nb + nc + nd == 0)
        return RT_OK;
    unsigned long long blocks = (na + nb + nc + nd + 255) / 256;
    blocks                    = blocks > 4096 ? 4096 : blocks;
    hipLaunchKernelGGL(rt::rt_zero4_kernel, dim3((unsigned) blocks), dim3(256), 0, stream, (unsigned long long *) a, na,
                       (unsigned long long *) b, nb, (unsigned long long *) c, nc, (unsigned long long *) d, nd);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int launch_zero3(hipStream_t stream, void *a, size_t a_bytes, void *b, size_t b_bytes, void *c, size_t c_bytes)
{
    // (8-byte words: the image and I_ang are doubles, DevCtl is 8-byte aligned and sized)
    const unsigned long long na = a ? a_bytes / 8 : 0, nb = b ? b_bytes / 8 : 0, nc = c ? c_bytes / 8 : 0;
    if (na + nb + nc == 0)
        return RT_OK;
    unsigned long long blocks = (na + nb + nc + 255) / 256;
    blocks                    = blocks > 4096 ? 4096 : blocks;
    hipLaunchKernelGGL(rt::rt_zero_kernel, dim3((unsigned) blocks), dim3(256), 0, stream, (unsigned long long *) a, na,
                       (unsigned long long *) b, nb, (unsigned long long *) c, nc);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int launch_tan(const rt_ray *rays_dev, unsigned long long n, float *sxy_dev, hipStream_t stream)
{
    if (n == 0)
        return RT_OK;
    hipLaunchKernelGGL(rt::rt_tan_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, rays_dev, n, sxy_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int launch_seed_tab(const rt::DevSeed &sd, const rt::DevRays &R, size_t n_points, double *sf, unsigned char *sin)
{
    hipLaunchKernelGGL(rt::rt_seed_tab_kernel, dim3((unsigned) ((n_points + 255) / 256)), dim3(256), 0, nullptr, sd, R, sf, sin);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int launch_selftest(unsigned long long *counts_dev)
{
    hipLaunchKernelGGL(rt::rt_selftest_kernel, dim3(1024), dim3(256), 0, nullptr, counts_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// A run whose frequency pass reported failing rays (error -2 / -3) has deposited them: repeat the pass
// over the same march records, first integrating without depositing to mark the failing rays, then
// depositing all others (DevParams::safe).  Leaves image / I_ang as the CPU loop leaves them
// (RayTraceImageCPU.cpp:29-36) and the failure report as the first pass of the repeat gives it.
int plan_repeat_checked(rt_hip_plan *p)
{
    hipStream_t stream = p->last_stream;
    const RecordSet &R    = p->last_records;
    const size_t bad_word = R.bad_word();
    if (p->bad_rays < (size_t) p->n_rays * bad_word || !p->bad_dev) {
        (void) hipFree(p->bad_dev);
        p->bad_dev = nullptr;
        HIP_TRY(dev_malloc((void **) &p->bad_dev, (size_t) p->n_rays * bad_word + 16));
        p->bad_rays = (size_t) p->n_rays * bad_word;
    }
    p->bad_word = bad_word;
    HIP_TRY(hipMemsetAsync(p->bad_dev, 0, (size_t) p->n_rays * bad_word, stream));
    HIP_TRY(hipMemsetAsync(&p->ctl->failure_code, 0, sizeof(unsigned), stream));
    HIP_TRY(hipMemsetAsync(&p->ctl->n_failed, 0, sizeof(unsigned), stream));
    HIP_TRY(hipMemsetAsync(p->ctl->seed_code, 0, sizeof(p->ctl->seed_code), stream));
    HIP_TRY(hipMemsetAsync(p->ctl->len_code, 0, sizeof(p->ctl->len_code), stream));
    HIP_TRY(hipMemsetAsync(p->ctl->seed_len_code, 0, sizeof(p->ctl->seed_len_code), stream));
    HIP_TRY(hipMemsetAsync(p->ctl->rec_code, 0, sizeof(p->ctl->rec_code), stream));
    HIP_TRY(hipMemsetAsync(p->ctl->rec_len_code, 0, sizeof(p->ctl->rec_len_code), stream));
    HIP_TRY(hipMemsetAsync(p->ctl->next_tile_f, 0, sizeof(p->ctl->next_tile_f), stream));
    const bool step = p->last_step; // a step run: the step kernel honours the same marks, E_v and nf start over
    RunFacts f          = run_facts(p);
    f.step_on           = step; // (the run that is repeated decides, not what the plan has been switched to since)
    f.path_on = f.spectra_on = false;
    f.scan_on           = R.scan();
    f.n_seed            = R.n_seed;
    const Tuning t      = read_tuning();
    const PassKind kind = pass_kind(f); // (of record_set(f), which is R again)
    int rc              = launch_pass(p, f, t, kind, stream, 1, p->bad_dev);
    if (rc == RT_OK) {
        if (step && p->last_step_lent) { // (the caller's buffers: exactly the K and nx * ny doubles that are the run's)
            HIP_TRY(hipMemsetAsync(p->step.E_v, 0, (size_t) p->P.K * sizeof(double), stream));
            HIP_TRY(hipMemsetAsync(p->step.nf, 0, (size_t) p->P.beam.nx * (size_t) p->P.beam.ny * sizeof(double), stream));
        } else if (step && R.n_rec() > 0) // (every record, its I_ang included, is in the one allocation)
            HIP_TRY(hipMemsetAsync(p->recs_dev, 0, p->recs_doubles * sizeof(double), stream));
        else if (step)
            HIP_TRY(hipMemsetAsync(p->step_dev, 0, p->step_doubles * sizeof(double), stream));
        else if (!p->P.exclusive)
            HIP_TRY(hipMemsetAsync(p->last_image, 0, p->n_image * sizeof(double), stream));
        HIP_TRY(hipMemsetAsync(p->last_iang, 0, p->n_iang * sizeof(double), stream));
        HIP_TRY(hipMemsetAsync(p->ctl->next_tile_f, 0, sizeof(p->ctl->next_tile_f), stream));
        rc = launch_pass(p, f, t, kind, stream, 2, p->bad_dev);
    }
    if (rc != RT_OK)
        return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

RecordSet plan_record_set(const rt_hip_plan *p) { return record_set(run_facts(p)); }
RowSet plan_row_set(const rt_hip_plan *p) { return row_set(run_facts(p)); }

// ---- the steps of a run --------------------------------------------------------------------------------------------
// step 2's device query: what hipOccupancyMaxActiveBlocksPerMultiprocessor says of the march instance `s` names (its LDS
// attribute raised first, as the launch will need it anyway)
static int march_occupancy(const rt_hip_plan *p, const RunShape &s, int &rc)
{
    const march_fn kernel = march_kernel(s.lds_tab, s.bounded, s.mode, s.opt);
    int per_cu            = 0;
    rc = allow_lds(reinterpret_cast<const void *>(kernel), p->device, s.mlds, p->lds_limit);
    if (rc == RT_OK) {
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int) s.bthr, s.mlds);
        if (e != hipSuccess)
            rc = fail_hip(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor(march kernel)", __FILE__, __LINE__);
    }
    return per_cu;
}

// step 3: the buffers the run writes -- march records, path tracer outputs, the spectra set of this run, the links of a
// one-launch run's tile lists -- kept while they are large enough
static int ensure_buffers(rt_hip_plan *p, const RunShape &s, hipStream_t stream)
{
    const size_t need = rt::rec_bytes(p->n_rays, p->P.rec_stride); // (whole 64-ray tiles: the records are tile-wise)
    if (need > p->rec_bytes || !p->rec) {
        plan_quiesce(p);
        pool_free(p->device, p->rec);
        p->rec = nullptr;
        HIP_TRY(pool_alloc(p->device, (void **) &p->rec, need ? need : 16));
        p->rec_bytes = need;
    }
    p->P.rec = p->rec;
    if ((p->scan_on && p->step_on) || p->lspec_on) { // a length scan or length spectra: the boundary states of the march, from the plan's pool while the mode is on
        const size_t bnd = rt::scan_bnd_bytes(p->n_rays, p->P.L);
        if (bnd > p->scan_bnd_bytes || !p->scan_bnd) {
            plan_quiesce(p);
            pool_free(p->device, p->scan_bnd);
            p->scan_bnd       = nullptr;
            p->scan_bnd_bytes = 0;
            HIP_TRY(pool_alloc(p->device, (void **) &p->scan_bnd, bnd ? bnd : 16));
            p->scan_bnd_bytes = bnd;
        }
    }
    if (p->path_on) {
        const size_t n2 = (size_t) p->P.L * RT_N_SUB + 1;
        if (p->path_rays != (size_t) p->n_rays || !p->path_dev) {
            (void) hipFree(p->path_dev);
            (void) hipFree(p->path_err);
            p->path_dev = nullptr;
            p->path_err = nullptr;
            HIP_TRY(dev_malloc((void **) &p->path_dev, (size_t) p->n_rays * n2 * 3 * sizeof(float) + 16));
            HIP_TRY(hipMalloc((void **) &p->path_err, (size_t) p->n_rays * sizeof(int32_t) + 16));
            p->path_rays = (size_t) p->n_rays;
        }
        HIP_TRY(hipMemsetAsync(p->path_dev, 0, (size_t) p->n_rays * n2 * 3 * sizeof(float), stream));
        HIP_TRY(hipMemsetAsync(p->path_err, 0, (size_t) p->n_rays * sizeof(int32_t), stream));
        p->P.path     = p->path_dev;
        p->P.path_err = p->path_err;
    }
    // the rows of a per-ray spectra run (rt_records.h, RowSet: the blocks of THIS run, with the strides of its ray count), no
    // zeroing: the kernel writes every element.  Iv [n_blocks][n][K] | ray2 | err [n_blocks][n], each part padded by 16 bytes
    // and, the last apart, to 256
    const RowSet R = row_set(run_facts(p));
    const size_t n = (size_t) p->n_rays, rows = n * (size_t) R.n_blocks();
    if (R.any() && !R.lengths()) {
        // spectra mode: the buffers of this run's set, kept while they are large enough (and then laid out as they were made);
        // ray2 [n] serves every block, its part has room for as many rows as the others
        rt::SpecOut &o = p->spec[p->spec_sel];
        if (p->spec_rays[p->spec_sel] < rows || !o.Iv) {
            plan_quiesce(p);
            (void) hipFree(o.Iv);
            o = {};
            p->spec_rays[p->spec_sel] = 0;
            const size_t iv_bytes = align_up(rows * (size_t) p->P.K * sizeof(double) + 16, 256), r2_bytes = align_up(rows * sizeof(rt_ray) + 16, 256);
            unsigned char *b = nullptr;
            HIP_TRY(dev_malloc((void **) &b, iv_bytes + r2_bytes + rows * sizeof(int32_t) + 16));
            o.Iv   = reinterpret_cast<double *>(b);
            o.ray2 = reinterpret_cast<rt_ray *>(b + iv_bytes);
            o.err  = reinterpret_cast<int32_t *>(b + iv_bytes + r2_bytes);
            p->spec_rays[p->spec_sel] = rows;
        }
    }
    if (R.lengths()) {
        // length spectra: one allocation from the pool, kept while it is large enough and laid out anew by every run; ray2
        // [L][n]; a run that cannot have it fails with RT_ERR_NOMEM
        const size_t iv_bytes = align_up(rows * (size_t) p->P.K * sizeof(double) + 16, 256), r2_bytes = align_up((size_t) R.n_ray2_blocks() * n * sizeof(rt_ray) + 16, 256);
        const size_t need_ls  = iv_bytes + r2_bytes + rows * sizeof(int32_t) + 16;
        if (need_ls > p->lspec_bytes || !p->lspec_dev) {
            plan_quiesce(p);
            pool_free(p->device, p->lspec_dev);
            p->lspec_dev   = nullptr;
            p->lspec_bytes = 0;
            p->lspec       = {};
            const hipError_t e = pool_alloc(p->device, (void **) &p->lspec_dev, need_ls);
            if (e == hipErrorOutOfMemory) {
                (void) hipGetLastError();
                fail_arg("length spectra: the rows of every length (L n K 8 bytes) do not fit into device memory");
                return RT_ERR_NOMEM;
            }
            HIP_TRY(e);
            p->lspec_bytes = need_ls;
        }
        p->lspec.Iv   = reinterpret_cast<double *>(p->lspec_dev);
        p->lspec.ray2 = reinterpret_cast<rt_ray *>(p->lspec_dev + iv_bytes);
        p->lspec.err  = reinterpret_cast<int32_t *>(p->lspec_dev + iv_bytes + r2_bytes);
    }
    if (s.kind != RUN_TWO_KERNELS && (p->tile_next_n < s.tile_links || !p->tile_next)) {
        plan_quiesce(p);
        pool_free(p->device, p->tile_next);
        p->tile_next = nullptr;
        HIP_TRY(pool_alloc(p->device, (void **) &p->tile_next, s.tile_links * sizeof(unsigned) + 16));
        p->tile_next_n = s.tile_links;
    }
    return RT_OK;
}

// what the kernels of this run get: the plan's parameter block with the numbers of this run in it (of its one march
// launch; launch_march adjusts the copy per upload slice)
static rt::DevParams run_params(const rt_hip_plan *p, const RunShape &s)
{
    rt::DevParams P = p->P;
    P.chunk       = s.chunk;
    P.park        = s.park;
    P.path_on     = p->path_on ? 1u : 0u;
    P.spin_limit  = s.spin_limit;
    P.no_skip     = s.no_skip;
    P.late_first  = s.late_first;
    P.late_waves  = s.late_waves;
    P.late_chunks = s.late_chunks;
    P.ray_begin   = 0;
    P.ray_end     = (unsigned) p->n_rays;
    P.launch_id   = 0;
    if (s.opt & rt::MARCH_OPT_SCAN) { // the scan instance of the march reads the boundary buffer's address here
        const unsigned long long b = (unsigned long long) (uintptr_t) p->scan_bnd;
        P.pad_march[0]             = (unsigned) (b & 0xffffffffull);
        P.pad_march[1]             = (unsigned) (b >> 32);
    }
    return P;
}

// step 5, the whole path in one launch: the march's parameter block, the argument block of the frequency (or step) pass
// behind it, the links and the layout
static int launch_one(rt_hip_plan *p, const RunFacts &f, const RunShape &s, const rt::DevParams &P, hipStream_t stream)
{
    const rt::FreqKArg fa = freq_args(p, true, s.nslot, s.fetch_shift, PassRun{ 0, f.n_tiles, 0, 0, nullptr });
    if (s.kind == RUN_STEP_ONE_LAUNCH) {
        // the step kernel's argument block as launch_pass fills it (lent buffers and the run's I_ang through p->step and freq_args)
        rt::FusedStepKArg sa;
        memset(&sa, 0, sizeof(sa));
        sa.P           = P;
        sa.S           = pass_args<rt::StepKArg>(fa);
        sa.S.out       = p->step;
        sa.tile_next   = p->tile_next;
        sa.lay         = s.lay;
        return launch(p, fused_step_kernel(s.bounded, f.s6(), s.opt), s.fgrid, s.bthr, s.flds, stream, sa);
    }
    rt::FusedKArg a;
    a.P         = P;
    a.F         = fa;
    a.tile_next = p->tile_next;
    a.lay       = s.lay;
    return launch(p, fused_kernel(s.bounded, f.s6(), s.maxq, s.emis, s.opt), s.fgrid, s.bthr, s.flds, stream, a);
}

// step 5, the march as a kernel of its own: one launch per upload slice of a ray list that is still on the host, each
// behind the synchronous copy of its slice
static int launch_march(rt_hip_plan *p, const RunShape &s, rt::DevParams &P, hipStream_t stream)
{
    const march_fn kernel = march_kernel(s.lds_tab, s.bounded, s.mode, s.opt);
    for (unsigned c = 0; c < s.n_launch && s.grid > 0 && !(P.debug & 2u); c++) {
        const unsigned long long b = p->n_rays * c / s.n_launch, e = p->n_rays * (c + 1) / s.n_launch;
        if (p->host_rays) {
            HIP_TRY(hipMemcpy(p->rays_dev + b, p->host_rays + b, (size_t) (e - b) * sizeof(rt_ray), hipMemcpyHostToDevice));
            // Helper.h:409-410 for every ray of the slice, at full lane occupancy, before its march
            if (tan_mode(p->device) == 2) { // this host's tanf is not the restated one: its own values
                std::vector<float> h((size_t) (e - b) * 2);
                host_tangents(p->host_rays + b, (size_t) (e - b), h.data());
                HIP_TRY(hipMemcpy(p->tan_dev + 2 * b, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
            } else {
                hipLaunchKernelGGL(rt::rt_tan_kernel, dim3((unsigned) ((e - b + 255) / 256)), dim3(256), 0, stream,
                                   p->rays_dev + b, (unsigned long long) (e - b), p->tan_dev + 2 * b);
                HIP_TRY(hipGetLastError());
            }
        }
        if (s.n_launch > 1) // rays reserved per counter fetch, for this slice
            P.chunk = march_chunk(e - b, s.grid, s.bthr);
        P.ray_begin = (unsigned) b;
        P.ray_end   = (unsigned) e;
        P.launch_id = c;
        const int rc = launch(p, kernel, s.grid, s.bthr, s.mlds, stream, P);
        if (rc != RT_OK)
            return rc;
    }
    return RT_OK;
}

// step 6: the second pass of a two-kernel run
static int launch_second(rt_hip_plan *p, const RunFacts &f, const Tuning &t, const rt::DevParams &P, hipStream_t stream)
{
    const PassKind kind = pass_kind(f);
    if (kind == PASS_PATH) { // the tracer replaces the frequency / deposit kernel: no image is produced
        if (p->n_rays) {
            hipLaunchKernelGGL(rt::rt_path_kernel, dim3((unsigned) ((p->n_rays + 255) / 256)), dim3(256), 0, stream, P);
            HIP_TRY(hipGetLastError());
        }
        return RT_OK;
    }
    if (!spectra_pass(kind) && (f.debug & 1u)) // (profiling: the march alone)
        return RT_OK;
    return launch_pass(p, f, t, kind, stream);
}

// One run on a queue: the march (persistent lanes) -> one record per ray -> the frequency pass, as ONE launch
// (rt_fused.hip) where that applies, as two kernels otherwise (or the path tracer in place of the frequency kernel).
// What the run looks like is run_shape's decision (rt_run_shape.h); nothing per-launch is written into the plan's
// parameter block.
int plan_launch_run(rt_hip_plan *p, hipStream_t stream)
{
    // the kernels index rays with 32 bits and round the ray count up to whole chunks of at most 4096 rays
    if (p->n_rays > (unsigned long long) MAX_LIST_RAYS)
        return fail_arg("more than 2^32 - 4096 rays in one run");
    const RunFacts f = run_facts(p);
    const Tuning t   = read_tuning();
    int rc           = RT_OK;
    const RunShape s = run_shape(f, t, [&](const RunShape &m) { return march_occupancy(p, m, rc); });
    if (rc != RT_OK)
        return rc;
    p->last_march_inst = s.last_march_inst;
    if ((rc = ensure_buffers(p, s, stream)) != RT_OK)
        return rc;
    HIP_TRY(hipEventRecord(p->ev0, stream));
    p->last_fused  = false;
    rt::DevParams P = run_params(p, s);
    const bool one = s.kind != RUN_TWO_KERNELS;
    if ((rc = one ? launch_one(p, f, s, P, stream) : launch_march(p, s, P, stream)) != RT_OK)
        return rc;
    p->host_rays = nullptr; // consumed: the list is on the device now
    HIP_TRY(hipEventRecord(p->evm, stream));
    if (!one && (rc = launch_second(p, f, t, P, stream)) != RT_OK)
        return rc;
    HIP_TRY(hipEventRecord(p->ev1, stream));
    p->last_fused = one;
    return RT_OK;
}

} // namespace rtr

extern "C" {

// What a run of these facts would look like, by the very functions plan_launch_run calls; no device call.
int rt_hip_debug_run_shape(const rt_hip_run_facts *facts, rt_hip_run_shape *out)
{
    if (!facts || !out || facts->size != sizeof(rt_hip_run_facts) || out->size != sizeof(rt_hip_run_shape))
        return fail_arg("rt_hip_debug_run_shape: NULL argument or a size field that is not this library's sizeof");
    if (facts->cu_count < 1 || facts->lds_limit == 0)
        return fail_arg("rt_hip_debug_run_shape: cu_count < 1 or lds_limit == 0");
    RunFacts f;
    f.cu_count        = facts->cu_count;
    f.lds_limit       = (size_t) facts->lds_limit;
    f.n_rays          = facts->n_rays;
    f.n_tiles         = facts->n_tiles;
    f.blob_bytes      = (size_t) facts->blob_bytes;
    f.K               = facts->K;
    f.Kp              = facts->Kp;
    f.L               = facts->L;
    f.n_iang          = (size_t) facts->n_iang;
    f.rays_per_pixel  = facts->rays_per_pixel;
    f.n_seed          = facts->n_seed;
    f.c_h3            = facts->c_h3;
    f.march_prune     = facts->march_prune;
    f.method          = facts->method;
    f.safe            = facts->safe;
    f.debug           = facts->debug;
    f.use_emis        = facts->use_emis != 0;
    f.own_cells       = facts->own_cells != 0;
    f.exclusive       = facts->exclusive != 0;
    f.path_on         = facts->path_on != 0;
    f.spectra_on      = facts->spectra_on != 0;
    f.step_on         = facts->step_on != 0;
    f.step_one_launch = facts->step_one_launch != 0;
    f.probe_on        = facts->probe_on != 0;
    f.has_ray_list    = facts->has_ray_list != 0;
    f.host_rays       = facts->host_rays != 0;
    f.tables_bounded  = facts->tables_bounded != 0;
    f.ntest_proven    = facts->ntest_proven != 0;
    f.gv_has_nan      = facts->gv_has_nan != 0;
    f.scan_on         = facts->scan_on != 0;
    // (length spectra travel as value 2 of spectra_on: the struct keeps its layout, include/rt_hip.h)
    f.length_spectra_on = facts->spectra_on == 2;
    f.spectra_on        = facts->spectra_on != 0 && facts->spectra_on != 2;
    const Tuning t    = read_tuning();
    const RunShape s  = run_shape(f, t, [&](const RunShape &) { return facts->occupancy_per_cu; });
    const unsigned size = out->size;
    memset(out, 0, sizeof(*out));
    out->size            = size;
    out->kind            = (int) s.kind;
    out->lds_tab         = s.lds_tab;
    out->n_launch        = s.n_launch;
    out->bthr            = s.bthr;
    out->mode            = s.mode;
    out->bounded         = s.bounded;
    out->opt             = s.opt;
    out->last_march_inst = s.last_march_inst;
    out->mlds            = s.mlds;
    out->grid            = s.grid;
    out->chunk           = s.chunk;
    out->park            = s.park;
    out->spin_limit      = s.spin_limit;
    out->no_skip         = s.no_skip;
    out->late_first      = s.late_first;
    out->late_waves      = s.late_waves;
    out->late_chunks     = s.late_chunks;
    out->occupancy_asked = s.occupancy_asked;
    out->key_s6          = f.s6();
    out->key_emis        = f.use_emis;
    out->key_excl        = f.use_emis && f.exclusive;
    if (s.kind != RUN_TWO_KERNELS) { // the one launch; its frequency (or step) phase stands where the second pass stands
        out->maxq            = s.maxq;
        out->nslot           = s.nslot;
        out->off_exp         = s.lay.off_exp;
        out->off_iang        = s.lay.off_iang;
        out->off_ctl         = s.lay.off_ctl;
        out->off_rem         = s.lay.off_rem;
        out->off_nodes       = s.lay.off_nodes;
        out->off_buf         = s.lay.off_buf;
        out->node_cap        = s.lay.node_cap;
        out->n_free          = s.lay.n_free;
        out->per_wave        = s.lay.per_wave;
        out->split           = s.lay.split;
        out->k_part          = s.lay.k_part;
        out->n_consumers     = s.lay.n_consumers;
        out->consumers_first = s.lay.consumers_first;
        out->flds            = s.flds;
        out->tile_links      = s.tile_links;
        out->fgrid           = s.fgrid;
        out->pass_kind       = s.kind == RUN_STEP_ONE_LAUNCH ? (int) PASS_STEP : (int) PASS_FREQ;
        out->pass_wg_waves   = (int) (s.bthr / 64);
        out->pass_in_lds     = 1;
        out->pass_nslot      = s.nslot;
        out->pass_lds        = s.flds;
        out->pass_grid       = s.fgrid;
        out->pass_fetch_shift = s.fetch_shift;
        return RT_OK;
    }
    const PassKind kind   = pass_kind(f);
    const PassShape ps    = pass_shape(kind, f, t);
    out->pass_kind        = (int) kind;
    out->pass_wg_waves    = ps.wg_waves;
    out->pass_in_lds      = ps.in_lds;
    out->pass_nslot       = ps.nslot;
    out->pass_lds         = ps.lds;
    out->pass_grid        = ps.grid;
    out->pass_fetch_shift = ps.fetch_shift;
    return RT_OK;
}

#ifdef RT_WAVETIMES
// diagnostic build only: wave start / dry / end times of the LAST march launch (100 MHz ticks), then reset
int rt_hip_debug_wavetimes(unsigned long long *summary8, unsigned long long *end8192, unsigned long long *dry8192)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(summary8, HIP_SYMBOL(rt::g_wt), 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyFromSymbol(end8192, HIP_SYMBOL(rt::g_wt_end), 8192 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyFromSymbol(dry8192, HIP_SYMBOL(rt::g_wt_dry), 8192 * sizeof(unsigned long long)));
    unsigned long long init[8] = { ~0ull, 0, ~0ull, 0, ~0ull, 0, 0, 0 };
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_wt), init, sizeof(init)));
    return RT_OK;
}
// the march trace of every wave (rt_march.hip: g_wt_trace), then cleared
int rt_hip_debug_wavetrace(unsigned long long *trace, int samples, unsigned *blocks)
{
    HIP_TRY(hipDeviceSynchronize());
    if (samples != rt::WT_TRACE)
        return fail_arg("rt_hip_debug_wavetrace: samples");
    if (blocks)
        HIP_TRY(hipMemcpyFromSymbol(blocks, HIP_SYMBOL(rt::g_wt_blocks), sizeof(unsigned) * 8192 * rt::WT_TRACE * 6));
    HIP_TRY(hipMemcpyFromSymbol(trace, HIP_SYMBOL(rt::g_wt_trace), sizeof(unsigned long long) * 8192 * rt::WT_TRACE));
    void *sym = nullptr;
    HIP_TRY(hipGetSymbolAddress(&sym, HIP_SYMBOL(rt::g_wt_trace)));
    HIP_TRY(hipMemset(sym, 0, sizeof(unsigned long long) * 8192 * rt::WT_TRACE));
    return RT_OK;
}
// time in tile_publish per wave (rt_march.hip: g_wt_pub, g_wt_vm), then cleared
int rt_hip_debug_publish(unsigned long long *pub4, unsigned long long *vm)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(pub4, HIP_SYMBOL(rt::g_wt_pub), sizeof(unsigned long long) * 8192 * 4));
    HIP_TRY(hipMemcpyFromSymbol(vm, HIP_SYMBOL(rt::g_wt_vm), sizeof(unsigned long long) * 8192));
    void *sym = nullptr;
    HIP_TRY(hipGetSymbolAddress(&sym, HIP_SYMBOL(rt::g_wt_pub)));
    HIP_TRY(hipMemset(sym, 0, sizeof(unsigned long long) * 8192 * 4));
    HIP_TRY(hipGetSymbolAddress(&sym, HIP_SYMBOL(rt::g_wt_vm)));
    HIP_TRY(hipMemset(sym, 0, sizeof(unsigned long long) * 8192));
    return RT_OK;
}
// ... and of the LAST frequency launch: times[6][8192] = {start, tables ready, first tile done, last tile done, where, tiles} per wave
int rt_hip_debug_freqtimes(unsigned long long *times, unsigned *n_waves)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(times, HIP_SYMBOL(rt::g_ft), 6 * 8192 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyFromSymbol(n_waves, HIP_SYMBOL(rt::g_ft_n), sizeof(unsigned)));
    const unsigned zero = 0;
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_ft_n), &zero, sizeof(zero)));
    return RT_OK;
}
#endif

#ifdef RT_INSTRUMENT
// diagnostic build only: loop iterations per ray of the last march (rays below 2^23)
int rt_hip_debug_ray_iters(unsigned short *out, unsigned long long n)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(rt::g_ray_iters), (size_t) n * sizeof(unsigned short)));
    return RT_OK;
}
#endif
#ifdef RT_INSTRUMENT
// diagnostic build only: read and clear the counters of the step-candidate pruning (rt_math.h, g_prune): wave-iterations
// of block [C] in which the division of h1 and those of h2 and h4 were executed, and wave-iterations of [C] in a pruning instance
int rt_hip_debug_prune_counters(unsigned long long *out4)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out4, HIP_SYMBOL(rt::g_prune), 4 * sizeof(unsigned long long)));
    unsigned long long z[4] = { 0 };
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_prune), z, sizeof(z)));
    return RT_OK;
}
#endif
#ifdef RT_TIMEBLOCKS
// diagnostic build only: read and clear the counters of the retirement of finished rays (rt_march.hip, g_retire)
int rt_hip_debug_retire_counters(unsigned long long *out4)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out4, HIP_SYMBOL(rt::g_retire), 4 * sizeof(unsigned long long)));
    unsigned long long z[4] = { 0 };
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_retire), z, sizeof(z)));
    return RT_OK;
}
#endif
#if defined(RT_INSTRUMENT) || defined(RT_TIMEBLOCKS)
// diagnostic builds only: read and clear the loop-occupancy / block-clock counters
int rt_hip_debug_counters(unsigned long long *out8)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out8, HIP_SYMBOL(rt::g_inst), 8 * sizeof(unsigned long long)));
    unsigned long long z[8] = { 0 };
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt::g_inst), z, sizeof(z)));
    return RT_OK;
}
#endif

} // extern "C"
