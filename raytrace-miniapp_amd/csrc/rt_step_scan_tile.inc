// rt_step_scan_tile.inc -- what the tile functions of the six scan passes of step mode do once per tile, ahead of their
// chunks: step_scan_tile, step_scan_seeds_tile, step_scan_ase_seeds_tile (forward: one record per length) and step_rscan_tile,
// step_rscan_seeds_tile, step_rscan_ase_seeds_tile (backward: one record per suffix).
//
// Fragments of a function body (rt_tile_rec.inc says why text); the includer defines which part it wants, in this order:
//   SCAN_TILE_HEAD      the constants of a tile, the per-ray preamble (rt_tile_ray.inc; the launch ray is not kept across
//                       the tile: what needs it loads it, a failing ray loads its own when it is reported), the early return
//                       of a tile without rays, the probe's flags and steps (those of the whole run), and the segment the
//                       ray escaped in.  Reads SF (= 0: slots at run time), H, hflags, C, tile, lane;
//                         SCAN_TILE_BACKWARD   the method (true / false: a scan takes one method only)
//                         SCAN_TILE_MARK       the word type of the marks of the checking repeat (FreqHot::bad)
//                       Declares L, S, K, Kp, n_rays, ridx, have, backward, rrec, rec, safe_check,
//                       safe_skip, probe_on, mark, what rt_tile_ray.inc declares, n_done, flags_steps, e_seg ((n_done - 1) / 3 + 1
//                       of the RecMeta; never escaped: L + 1).
//   SCAN_TILE_LAUNCH_FACTORS   forward with a seed set: per seed the seed factor at the launch ray, place_ray's arithmetic and
//                       order (Helper.h:523-533) -- on a forward ray grid the product of the seed's tabulated factors
//                       (RT_SEED_GRID_FACTOR), otherwise scan_seed_factor on the seed's DevSeed.  Reads Z->tabs, n_seed, NS;
//                         SCAN_TILE_ON_GRID    the launch rays are grid points (R.sf; Z->tabs.sf[0]: the tables of the seeds
//                                              exist on a forward ray grid, for all seeds or none)
//                       Declares f0_launch[NS].
//   SCAN_TILE_LAUNCH_PLACE     backward: the method deposits at the LAUNCH ray (RayTraceImageCPU.cpp:37-39), so pixel, angle
//                       cell and the runs of equal pixel (rt_wave_runs.inc) are the same for every record and are taken
//                       once: the last lane of a run owns the run's total of every record (a record's own depositing lanes
//                       are a subset of the run: the others add 0.0).  The probe's exit ray is that of the whole run,
//                       written as rt_step_kernel writes it: not under error -1.
//                         SCAN_TILE_PLACED     the ray takes its cells (!(fl & F_SKIP); true where the seed records take
//                                              a ray the march marked F_SKIP)
//                       Declares pix, ang, has_pix and what rt_wave_runs.inc declares.
//   SCAN_TILE_REC       the march record of the lane's ray (rt_tile_rec.inc; SF = 0: nothing to decode up front, every
//                       frequency's lineshape values are tested as they are read).  Declares what rt_tile_rec.inc declares, dv2.
#if defined(SCAN_TILE_HEAD)
const int L           = H.L;
const int S           = L * RT_N_SUB;
const int K           = H.K;
const int Kp          = H.Kp;
const unsigned n_rays = H.n_rays;
const unsigned ridx   = tile * WAVE + (unsigned) lane;
const bool have       = ridx < n_rays;
const bool backward   = SCAN_TILE_BACKWARD;
const unsigned rrec      = have ? ridx : 0u;
const unsigned char *rec = H.rec;
const bool safe_check = (hflags & FQ_SAFE_CHECK) != 0, safe_skip = (hflags & FQ_SAFE_SKIP) != 0;
const bool probe_on   = (hflags & FQ_PROBE) != 0;
SCAN_TILE_MARK *mark  = reinterpret_cast<SCAN_TILE_MARK *>(H.bad);
#define TILE_NEED_RAY false
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
if (__ballot(have) == 0ull)
    return;
if (have && probe_on) {
    C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
    C->probe.steps[ridx] = steps;
}
const int n_done           = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
const unsigned flags_steps = m.flags_steps; // (what the backward walks need of the final state, which they do not hold)
(void) flags_steps;
const int e_seg            = (fl & F_ESCAPED) ? (n_done > 0 ? (n_done - 1) / RT_N_SUB + 1 : 1) : L + 1;
#elif defined(SCAN_TILE_LAUNCH_FACTORS)
double f0_launch[NS];
#pragma unroll
for (int s = 0; s < NS; s++)
    f0_launch[s] = 0.0;
if (have) {
    if (!SCAN_TILE_ON_GRID) {
        rt_ray launch = ray;
        float ta, tb;
        load_ray(R, ridx, launch, ta, tb, false);
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (s < n_seed) {
                const DevSeed SD = load_cold(&Z->tabs.seed[s]);
                f0_launch[s]     = scan_seed_factor(SD, (double) launch.x, (double) launch.y, (double) launch.a, (double) launch.b);
            }
        }
    } else {
        RT_SEED_GRID_POINT(R, ridx)
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (s < n_seed) {
                const double *sf         = Z->tabs.sf[s];
                const unsigned char *sin = Z->tabs.sin[s];
                RT_SEED_GRID_FACTOR(f0_launch[s], Z->tabs.seed[s].f0, sf, sin)
            }
        }
    }
}
#elif defined(SCAN_TILE_LAUNCH_PLACE)
int pix = -1, ang = -1;
if (have) {
    const unsigned pf = (hflags & ~(unsigned) (FQ_HAS_SEED | FQ_PROBE)) | (err1 ? 0u : (hflags & (unsigned) FQ_PROBE));
    rt_ray launch     = ray;
    if (!(hflags & FQ_OWN_CELLS)) { // (own cells: the grid point is the placement, no coordinate is read)
        float ta, tb;
        load_ray(R, ridx, launch, ta, tb, false);
    }
    const Placed P = place_ray(pf, C, R, H.nx, backward, ridx, m, fl, launch);
    if (SCAN_TILE_PLACED) {
        pix = P.pix;
        ang = P.ang;
    }
}
const bool has_pix = pix >= 0;
#define RUNS_PIX pix
#define RUNS_DEPOSITS has_pix
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
(void) pix_prev;
#elif defined(SCAN_TILE_REC)
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
(void) gs;
(void) rs;
(void) off;
(void) all_small;
(void) all_regular;
(void) load_rows;
(void) gv_nan;
(void) exact_emis; // (the gain-only walks do not read it)
const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;
#else
#error "rt_step_scan_tile.inc: define SCAN_TILE_HEAD, SCAN_TILE_LAUNCH_FACTORS, SCAN_TILE_LAUNCH_PLACE or SCAN_TILE_REC"
#endif
