/*
 * rt_hip.h -- C ABI of the MI355X (gfx950) ray-trace imaging backend.
 *
 * This is the drop-in boundary for ONE path of the XRayTrace miniapp: the
 * back-end loop that RayTrace::create_image dispatches to
 *
 *     void RayTraceImage<Backend>Loop( int N, const EUV_beam_struct& beam,
 *         const ray_gain_struct* gain, const ray_seed_struct* seed, int method,
 *         const std::vector<ray_struct>& rays, double scale, double* image,
 *         double* I_ang, unsigned int& failure_code,
 *         std::vector<ray_struct>& failed_rays );
 *                                   (reference: src/RayTraceImage.cpp:47-75)
 *
 * Everything here is plain C: PODs, pointers and sizes.  No C++ types, no
 * exceptions, no torch types.  The C++ adapter that a reference maintainer
 * links (raytrace-miniapp_amd/host/RayTraceImageHip.cpp) flattens the
 * reference structs into these records; tests and bench.py bind the same
 * symbols through ctypes.  oracle/rt_oracle.c (test infrastructure only)
 * consumes the same records so that parity tests feed both sides one input.
 *
 * All host arrays are borrowed for the duration of a call and never cached
 * across calls (reference Readme.txt:43).
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_N_SUB 3         /* sub-segments per length (RayTraceImageHelper.h:31) */
#define RT_N_FAILED_MAX 32 /* failed rays reported back (RayTraceImageHelper.h:32) */
#define RT_N_SEED_MAX 2    /* seed beams of one step record (N_SEED_MAX, RayTraceStructures.h:15) */

/* Status codes returned by every entry point. */
enum {
    RT_OK            = 0,
    RT_ERR_ARG       = 1, /* inconsistent sizes / NULL where data is required   */
    RT_ERR_NO_DEVICE = 2, /* no usable gfx950 device                           */
    RT_ERR_HIP       = 3, /* a HIP runtime call failed (see rt_hip_last_error) */
    RT_ERR_NOMEM     = 4
};

/* One ray: position (cm) and angle (mrad).  Replaces ray_struct
 * (src/common/RayTraceImageHelper.h:36-41); same layout, 16 bytes. */
typedef struct rt_ray {
    float x, y, a, b;
} rt_ray;

/* The fields of EUV_beam_struct (src/RayTraceStructures.h:26-52) that the
 * path reads: the output (deposit) grid and the frequency weights. */
typedef struct rt_beam {
    int32_t nx, ny, na, nb, nv;
    double dx, dy, da, db, dz;
    const double *x;  /* [nx] */
    const double *y;  /* [ny] */
    const double *a;  /* [na] */
    const double *b;  /* [nb] */
    const double *dv; /* [nv] */
} rt_beam;

/* Plasma tables of one length.  Replaces ray_gain_struct
 * (src/RayTraceStructures.h:218-228).  n,g0,E0: [ix + iy*Nx];
 * gv: [k + (ix + iy*Nx)*Nv].  gv0 is never read on the path. */
typedef struct rt_gain {
    int32_t Nx, Ny, Nv;
    const double *x; /* [Nx] */
    const double *y; /* [Ny] */
    const double *n; /* [Nx*Ny] index of refraction */
    const float *g0; /* [Nx*Ny] line-centre gain */
    const float *E0; /* [Nx*Ny] line-centre emissivity, may be NULL */
    const float *gv; /* [Nx*Ny*Nv] normalised lineshape */
} rt_gain;

/* Separable seed profile.  Replaces ray_seed_struct
 * (src/RayTraceStructures.h:276-281). */
typedef struct rt_seed {
    int32_t dim[5];
    const double *x[5];
    const double *f[5];
    double f0;
} rt_seed;

/* Counters measured by the run (not assumed): SURVEY.md 8(d). */
typedef struct rt_stats {
    uint64_t n_rays;      /* rays traced                                        */
    uint64_t cell_steps;  /* iterations of the cell loop, Helper.h:463-504      */
    uint64_t n_escaped;   /* rays that left the plasma                          */
    uint64_t n_skipped;   /* rays whose frequency pass was provably all-zero    */
    float kernel_ms;      /* device time of the trace kernel(s), HIP events     */
    float total_ms;       /* H2D + kernels + D2H as seen by the host-pointer API*/
    float march_ms;       /* device time of the march kernel (rt_march_kernel)  */
    float freq_ms;        /* device time of the frequency kernel (rt_freq_kernel)*/
} rt_stats;

/* Number of usable devices; replaces cudaGetDeviceCount in the multi-GPU arm
 * (src/RayTraceImage.cpp:398-399).  Returns 0 when there is none. */
int rt_hip_device_count(void);

/* Text of the last HIP failure on this thread ("" if none). */
const char *rt_hip_last_error(void);

/* Known-answer test of the exact-arithmetic shortcuts of the march on the device itself
 * (no reference counterpart: the CPU code divides and takes square roots with the IEEE
 * operators, src/common/RayTraceImageHelper.h:73-89).  Evaluates the shortcut and the IEEE
 * sequence for every float of the shortcut's range (and a strided sample of all others) and
 * counts the values where they differ in any bit.  n_mismatch must come back 0. */
int rt_hip_selftest(int device, unsigned long long *n_checked, unsigned long long *n_mismatch);

/*
 * Host-pointer entry point: what RayTraceImageHipLoop calls.
 * Replaces RayTraceImageCudaLoop (src/RayTraceImageCuda.cu:145-221):
 * one packed upload, the trace kernel, one download.
 *   image  [nx*ny*nv], I_ang [na*nb]: overwritten with this call's result
 *          (create_image hands them over zeroed, RayTraceImage.cpp:271-274).
 *   failure_code: bit (-error) set for error -1/-2/-3 (Helper.h:47-56,
 *          RayTraceImageCPU.cpp:32-36); failed_rays receives at most
 *          max_failed rays, *n_failed the number stored.  Where more than RT_N_FAILED_MAX rays fail
 *          with error -2 / -3, the rays reported are the first RT_N_FAILED_MAX of them in list order
 *          (the ones RayTraceImageCPULoop pushes first), whatever order the device met them in.
 *   stats may be NULL.
 * A ray list that is the full tensor grid of four 1-D grids in create_image's order
 * (src/RayTraceImage.cpp:300-328) is recognised: the rays are then generated on the device
 * (rt_hip_plan_set_ray_grid) while host threads verify the list ray by ray, bit for bit; should the
 * verification fail the result is discarded and the list itself is uploaded and traced.  Lists of
 * 2^32 - 4096 rays or more are rejected (RT_ERR_ARG): the kernels index rays with 32 bits.
 * If failure_code comes back non-zero, image and I_ang hold exactly what RayTraceImageCPULoop leaves:
 * the failing rays deposit nothing (RayTraceImageCPU.cpp:29-36) -- the frequency pass is repeated in a
 * checking mode for such a run.
 * Two kinds of ray on which the reference's loops never end are reported as invalid rays (error -1) instead of
 * being marched: a ray that starts inside the plasma with a NaN position or direction, and -- for tables or a dz
 * outside the ranges rt_hip_plan_create verifies -- the rays of a wave that has marched 2^24 iterations without
 * taking a new ray (steps that do not advance: an infinite dz in a medium without refraction).
 */
int rt_hip_image_loop(int device, int N, const rt_beam *beam, const rt_gain *gain,
                      const rt_seed *seed, int method, const rt_ray *rays, size_t n_rays,
                      double scale, double *image, double *I_ang, unsigned int *failure_code,
                      rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats);

/*
 * All devices of the node in one call: what RayTraceImageHipMultiGPULoop calls.  Replaces the
 * "cuda-multigpu" arm of the dispatcher (src/RayTraceImage.cpp:389-405), which runs
 * RayTraceImageThreadLoop (:89-134: contiguous ray chunks, one host thread and one private full image
 * per device, images added on the host at join) and, for the assembly, stands where a multi-rank run
 * of the application uses MPI (src/MPI_helpers.h:29-38, intensity_step_struct::sum_reduce).
 *   One process, one host thread per device, the device bound INSIDE the worker (the reference binds it
 *   in the spawning thread, RayTraceImage.cpp:116), one RCCL communicator over the ndev devices
 *   (ncclCommInitAll, kept across calls like the queues; librccl is loaded on first use).
 *   ASE (method 1, no seed) with `rays` = the full tensor grid of the beam (recognised from the list
 *   itself and verified ray by ray): pixel-column tiles -- device d traces image columns d, d+ndev, ...
 *   from a ray grid generated on the device and holds a compact tile [ny][nx_d][nv]; the tiles and the
 *   I_ang partial sums travel to device 0 in ONE grouped ncclSend/ncclRecv gather (every peer over its
 *   own xGMI link), one kernel interleaves the columns and adds the I_ang parts, one download.
 *   Anything else (seeded mode, arbitrary ray lists): contiguous ray chunks, a full image per device,
 *   ncclReduce(sum, f64) to device 0, one download.
 * ndev <= 0: all devices.  ndev = 1 is a degenerate communicator (self send/recv) and gives the image of
 * rt_hip_image_loop.  Same outputs and error convention as rt_hip_image_loop; stats: counters summed,
 * times = maximum over devices, total_ms = wall time of the call.
 */
int rt_hip_multi_image_loop(int ndev, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed,
                            int method, const rt_ray *rays, size_t n_rays, double scale, double *image,
                            double *I_ang, unsigned int *failure_code, rt_ray *failed_rays, int max_failed,
                            int *n_failed, rt_stats *stats);

/* Host-only helper (no device needed): 1 if the list is exactly the tensor grid of four 1-D grids in
 * create_image's order (b fastest, then a, y, x; src/RayTraceImage.cpp:300-328) -- every ray compared
 * bit for bit -- with dims = {nx, ny, na, nb}; 0 otherwise.  This is the test the two entry points
 * above apply before they generate the rays on the device. */
int rt_hip_ray_list_grid_dims(const rt_ray *rays, size_t n_rays, int dims[4]);

/* How the last rt_hip_multi_image_loop / rt_hip_multi_step_loop of this thread was partitioned: 1 = pixel-column
 * tiles + gather, 2 = ray chunks + sum-reduce, 3 = strided ray grid + sum-reduce of the step record
 * (rt_hip_multi_step_loop only), 0 = none yet.  (Diagnostics and tests.) */
int rt_hip_multi_last_mode(void);

/* List-mode launch tangents (Helper.h:409-410) are computed on the device by a restatement of glibc
 * 2.35's float tanf; once per process that restatement is compared with the host's tanf on 8192 angles.
 * 1: they agree, the device computes the tangents; 2: they do not (another libm; or RT_HIP_TAN_ON_HOST
 * set): the host's tanf computes them on host threads, so that every ray starts as RayTraceImageCPULoop on
 * this host starts it.  Ray grids always use the host's tanf (na + nb values). */
int rt_hip_host_libm_mode(int device);

/* Device allocations -- never data -- are kept across calls (ray lists, tangents, march records;
 * Readme.txt:43 forbids caching data only).  This returns every parked block of every device to the
 * driver; RT_HIP_POOL_MAX_MB in the environment caps what may be parked (default 32768).  The host-pointer entry
 * points also park up to eight page-locked staging buffers (tables on their way up, small outputs on their way
 * down, at most 256 MB each); this call frees those too. */
void rt_hip_pool_trim(void);

/*
 * Device-resident plan: the same path with inputs already in HBM, so that a
 * caller (bench.py, the multi-GPU driver) can time and re-run the kernel and
 * hand the output buffers to RCCL without a host round trip.
 */
typedef struct rt_hip_plan rt_hip_plan;

/* Upload beam grids, gain tables and seed tables in one arena. */
int rt_hip_plan_create(rt_hip_plan **plan, int device, int N, const rt_beam *beam,
                       const rt_gain *gain, const rt_seed *seed, int method, double scale);

/* Explicit ray list (the Loop signature's `rays`). */
int rt_hip_plan_set_rays(rt_hip_plan *plan, const rt_ray *rays, size_t n_rays);

/* Ray list generated on the device from the four 1-D grids exactly as
 * RayTrace::create_image builds it (src/RayTraceImage.cpp:300-328):
 * ray t has ijkm = first + t*stride; m = ijkm % nb fastest, then a, y, x;
 * coordinates are the grids rounded to float.  count rays are generated. */
int rt_hip_plan_set_ray_grid(rt_hip_plan *plan, const double *gx, int ngx, const double *gy,
                             int ngy, const double *ga, int nga, const double *gb, int ngb,
                             int64_t first, int64_t stride, int64_t count);

/* Zero the outputs and run the trace on `stream` (a hipStream_t, may be
 * NULL = the default stream).  image_dev / iang_dev are device pointers owned
 * by the caller (e.g. torch tensors) or NULL to use the plan's own buffers.
 * Asynchronous with respect to the host. */
int rt_hip_plan_run(rt_hip_plan *plan, void *stream, double *image_dev, double *iang_dev);

/* Wait for the last run; copy results of the plan's own buffers to the host
 * (either pointer may be NULL), and report failures and counters. */
int rt_hip_plan_fetch(rt_hip_plan *plan, double *image, double *I_ang,
                      unsigned int *failure_code, rt_ray *failed_rays, int max_failed,
                      int *n_failed, rt_stats *stats);

/* Device time in ms of the trace kernel of the last run (HIP events recorded on
 * the run's stream around the launch).  Waits for that run to finish. */
int rt_hip_plan_kernel_ms(rt_hip_plan *plan, float *ms);

/* The same, split by kernel: the march kernel (rt_march_kernel) and the frequency /
 * deposit kernel (rt_freq_kernel) of the last run. */
int rt_hip_plan_kernel_times(rt_hip_plan *plan, float *march_ms, float *freq_ms);

/* 1 if the plan's last run took the whole path in ONE launch (march and frequency pass as two phases of the same
 * persistent waves, raytrace-miniapp_amd/csrc/rt_fused.hip -- the shape of the reference's own GPU kernel,
 * src/RayTraceImageCuda.cu:66-127, in behaviour only): march_ms is then the time of that launch and freq_ms 0.
 * Taken for the emission mode on the beam's own ray grid when the frequency pass fits into LDS beside the march
 * tables; RT_HIP_FUSED=2 in the environment keeps the two-kernel run. */
int rt_hip_plan_last_fused(rt_hip_plan *plan);

/* The instance of the march the plan's last run took, as bits: 1 = the short division sequences (tables and step
 * factor inside the ranges plan_create verifies; otherwise the generic instance, all other bits 0); 2 and 4 together =
 * the integrator step skips the division of the step candidate h1 where it cannot set the step, and its loop condition
 * goes without the |n - n0| < 0.05 test -- taken where plan_create has proved from the tables that the test holds;
 * 8 = the divisions of h2 and h4 are skipped likewise (launches of at least 8192 rays per compute unit).
 * RT_HIP_MARCH_PRUNE in the environment at plan creation: 0 keeps bits 2, 4 and 8 off, 2 sets bit 8 at every launch
 * size.  Every instance gives the same march records. */
int rt_hip_plan_last_march_instance(rt_hip_plan *plan);

/* What a run would look like on the device, decided from plain numbers: the function a run itself calls to choose its
 * kernels, grids, LDS layout and chunking (raytrace-miniapp_amd/csrc/rt_run_shape.h), without a plan, a device or any
 * device call -- so that the launch rules can be tested on a machine that has no GPU.  The RT_HIP_* tuning knobs are read
 * from the environment exactly as a run reads them.  Both structs start with their own sizeof in `size` (set it in both
 * before the call); NULL, a wrong size, cu_count < 1 or lds_limit == 0 fail with an argument error.
 * facts: what a run takes from its plan.  rays_per_pixel = nga * ngb of the ray grid (0: a list); has_ray_list: the rays
 * are a list on the device; host_rays: the list is still on the host (rt_hip_image_loop); occupancy_per_cu stands for the
 * one device query a run makes (resident work-groups of the march instance per compute unit), consulted where a run
 * consults the device and nowhere else -- occupancy_asked says whether it was. */
typedef struct rt_hip_run_facts {
    unsigned size;
    int cu_count;
    unsigned long long lds_limit, n_rays, blob_bytes, n_iang;
    unsigned n_tiles;
    int K, Kp, L, rays_per_pixel, n_seed, march_prune, method;
    float c_h3;
    unsigned safe, debug;
    int use_emis, own_cells, exclusive, path_on, spectra_on, step_on, step_one_launch, probe_on, has_ray_list, host_rays,
        tables_bounded, ntest_proven, gv_has_nan;
    int occupancy_per_cu;
    int scan_on; /* a length scan (rt_hip_plan_enable_length_scan): the scan march and pass_kind 5, one record per length 1 .. L;
                    with method == 1 the suffix scan (rt_hip_plan_enable_suffix_scan): the backward scan march and pass_kind 9 */
} rt_hip_run_facts;
/* spectra_on = 2 stands for length spectra (rt_hip_plan_enable_length_spectra; any other non-zero value: spectra mode): the
 * scan march of the plan's method and pass_kind 12, with the LDS of the spectra pass.  The struct keeps its layout and still
 * ends with scan_on: the mode is a value of the fact that names the per-ray spectra, not a member of its own.  (Before length
 * spectra existed every non-zero spectra_on, 2 included, was spectra mode: a caller that wrote 2 for "on" now gets this.) */
/* kind: 0 = march and second pass as two kernels, 1 = the image run in one launch, 2 = the step run in one launch.
 * The march (of a one-launch run: its march phase): lds_tab (tables in LDS) ... late_chunks; bounded, mode, opt and
 * lds_tab name its instance, last_march_inst is what rt_hip_plan_last_march_instance would report.  chunk is that of a
 * run of one march launch; with n_launch > 1 every upload slice takes the same rule on its own rays.
 * maxq ... fgrid: a one-launch run only (else 0) -- the layout of its work-group in LDS (off_*, node_cap, n_free,
 * per_wave in doubles, split, k_part, n_consumers, consumers_first), its LDS bytes, the links of its tile lists and
 * its grid.  key_s6 / key_emis / key_excl pick the instance of the second pass.
 * pass_*: the second pass this run takes (pass_kind 0 frequency, 1 spectra, 2 step, 3 step of a seed set, 4 path
 * tracer: all zero, 5 step of a length scan, 6 step of a length scan with scan seeds (scan_on, n_seed > 0: one record per
 * seed and length), 12 length spectra (spectra_on = 2), 13 / 14 spectra mode / length spectra with spectra seeds (spectra_on = 1 / 2
 * with n_seed > 0), 15 spectra mode of an emission plan with ASE seeds (spectra_on = 1, use_emis, n_seed > 0); pass_lds above lds_limit: the run is refused); for a one-launch run the frequency (step) phase of that launch. */
typedef struct rt_hip_run_shape {
    unsigned size;
    int kind, lds_tab;
    unsigned n_launch, bthr;
    int mode, bounded, opt, last_march_inst;
    unsigned long long mlds;
    unsigned grid, chunk, park, spin_limit, no_skip, late_first, late_waves, late_chunks;
    int occupancy_asked;
    int maxq, nslot;
    unsigned off_exp, off_iang, off_ctl, off_rem, off_nodes, off_buf, node_cap, n_free, per_wave, split, k_part, n_consumers,
        consumers_first;
    unsigned long long flds, tile_links;
    unsigned fgrid;
    int key_s6, key_emis, key_excl;
    int pass_kind, pass_wg_waves, pass_in_lds, pass_nslot;
    unsigned long long pass_lds;
    unsigned pass_grid, pass_fetch_shift;
} rt_hip_run_shape;
int rt_hip_debug_run_shape(const rt_hip_run_facts *facts, rt_hip_run_shape *out);

/* Timing many back-to-back runs without waiting for each: keep the event triples of the last n_runs runs
 * (1 <= n_runs <= 4096); rt_hip_plan_ring_times waits for the last run and returns the kernel durations of
 * the most recent runs, oldest first (at most max_runs of them; *n_runs = how many).  Without a ring a plan
 * keeps the events of its last run only (rt_hip_plan_kernel_times). */
int rt_hip_plan_set_timing_ring(rt_hip_plan *plan, int n_runs);
int rt_hip_plan_ring_times(rt_hip_plan *plan, float *march_ms, float *freq_ms, int max_runs, int *n_runs);

/* Device pointers of the plan's own output buffers (for RCCL / torch views). */
double *rt_hip_plan_image_ptr(rt_hip_plan *plan);
double *rt_hip_plan_iang_ptr(rt_hip_plan *plan);

/* Per-ray march record of the last run, for parity tests against the oracle:
 * gvl/evl [n][L][3] float, ivl [n][L][3] int32, ray2 [n] rt_ray,
 * flags [n] (bit0 escaped, bit1 error -1, bit2 frequency pass skipped),
 * steps [n] cell-steps.  Any pointer may be NULL.  Requires
 * rt_hip_plan_enable_probe(plan, 1) before the run. */
int rt_hip_plan_enable_probe(rt_hip_plan *plan, int on);
int rt_hip_plan_fetch_probe(rt_hip_plan *plan, float *gvl, float *evl, int32_t *ivl,
                            rt_ray *ray2, uint32_t *flags, uint32_t *steps);

/* Emission (ASE) mode only.  By default the frequency pass advances
 *   Iv' = Iv + (e^gl - 1)(Iv + evl/gvl)
 * with the ratio taken once per sub-segment; the CPU (Helper.h:549-557) divides the two float32
 * products el/gl per frequency, which differs by one float rounding per term: image and I_ang agree
 * with RayTraceImageCPULoop to ~1e-8 rel-L2.  on = 1 runs the CPU's formula as written (~1e-14,
 * about twice the time of the frequency kernel).  No effect with a seed (gain-only mode). */
int rt_hip_plan_set_exact_emission(rt_hip_plan *plan, int on);

/* Step safety factor c of the integrator (`c` of RayTrace_calc_ray, Helper.h:381;
 * create_image always uses 0.5, RayTrace::calc_ray_path passes its own).  0 < c < 1. */
int rt_hip_plan_set_step_factor(rt_hip_plan *plan, double c);

/* Path tracer, replaces RayTrace::calc_ray_path (src/RayTraceImage.cpp:440-477): with it
 * enabled a run produces, instead of the image, for every ray the {x, y, I} triples at
 * the 3 (N-1) + 1 sub-segment boundaries -- exactly the `debug` array of
 * RayTrace_calc_ray (Helper.h:419-426, 505-511, 536-542, 559-566) -- and the ray's
 * return code (0, -1, -2, -3).  path: [n_rays][3 (N-1) + 1][3] floats, err: [n_rays]. */
int rt_hip_plan_enable_path(rt_hip_plan *plan, int on);
int rt_hip_plan_fetch_path(rt_hip_plan *plan, float *path, int32_t *err);

/* Spectra mode, replaces RayTrace::calc_ray (src/RayTraceImage.cpp:189-204) for every ray of the plan: with it
 * enabled a run produces, instead of the image, what calc_ray returns per ray -- the spectrum Iv [n_rays][K] (row
 * stride K), the exit ray ray2 [n_rays] and the return code err [n_rays] (0, -1, -2, -3; Helper.h:514-594, a negative
 * intensity wins over a NaN).  A ray with error -1 has a spectrum of zeros and ray2 = 0 (the reference leaves ray2
 * untouched there); the spectrum of a ray with error -2 / -3 is not meant to be read.  The march runs as in image mode
 * (two-kernel form), rt_spec_kernel (raytrace-miniapp_amd/csrc/rt_spec.hip) takes the place of the frequency kernel:
 * rt_hip_plan_kernel_times reports it as freq_ms.  rt_hip_plan_run takes no image buffers in this mode (NULL, NULL) and
 * rt_hip_plan_fetch no image pointers; it still reports failure_code (bit -err of every failing ray), the first failed
 * rays and the counters.  Works with ray lists and ray grids and together with the probe; together with the path tracer
 * it is RT_ERR_ARG.  Any pointer of fetch_spectra may be NULL; it copies the rows of the last RUN -- as many as that run had
 * rays, whatever ray set the plan has been given since.  spectra_ptr: device pointer of Iv of the last run (valid
 * until the next run or change of the ray set), for torch views.  (Which blocks of rows a run of either spectra mode leaves,
 * and what an index of the accessors below means: the table of RowSet, raytrace-miniapp_amd/csrc/rt_records.h.) */
int rt_hip_plan_enable_spectra(rt_hip_plan *plan, int on);
int rt_hip_plan_fetch_spectra(rt_hip_plan *plan, double *Iv, rt_ray *ray2, int32_t *err);
double *rt_hip_plan_spectra_ptr(rt_hip_plan *plan);

/* Length spectra: RayTrace::calc_ray for every ray of the plan at EVERY plasma length n = 2 .. N, from ONE march.  A mode
 * of its own beside spectra mode.  With it on a run marches once, with the scan instance of the march (the one a length
 * scan or a suffix scan takes: rt_hip_plan_last_march_instance carries its bit), and rt_spec_scan_kernel
 * (raytrace-miniapp_amd/csrc/rt_spec_scan.hip) leaves per ray and n what calc_ray returns on the sub-problem of n lengths
 * -- gain[0 .. n-1] on a forward plan (method 2), gain[0] and the LAST n - 1 lengths on a backward plan (method 1): the
 * spectrum Iv [K], the exit ray ray2 and the code err (0, -1, -2, -3; a negative intensity wins over a NaN).  Rows follow
 * spectra mode: error -1 gives a row of zeros and ray2 = 0, a row that is all zero on the CPU is all zero here, the
 * spectrum of a -2 / -3 row is not meant to be read.  In gain-only mode and with rt_hip_plan_set_exact_emission every
 * value is the double a spectra-mode plan of the sub-problem computes; in the default emission mode the two differ as the
 * records of a scan differ from a step plan's (the choice of the update is taken per sub-segment here).
 * enable_length_spectra(on != 0): 3 <= N and N - 1 <= RT_N_SCAN_MAX, and none of step mode, spectra mode, the path tracer,
 *   a length or suffix scan, a seed set, ASE seeds or the seeds of a scan may be on -- each is RT_ERR_ARG with its own
 *   text; the call settles the last run first.  While the mode is on each of those switches and installers is RT_ERR_ARG.
 *   on = 0 restores the plan exactly (the boundary states and the rows go back to the pool).  Seeded and emission plans,
 *   ray lists and ray grids (first / stride included), exact emission, the probe (of the whole run), the timing ring,
 *   rt_hip_plan_set_step_factor and rt_hip_plan_update_gain / _dev work as in spectra mode; an update keeps the mode.
 *   rt_hip_plan_set_step_one_launch is accepted and the run keeps two kernels (rt_hip_plan_last_fused is 0,
 *   rt_hip_plan_kernel_times reports the pass as freq_ms).
 * rt_hip_plan_run takes (NULL, NULL) in this mode and rt_hip_plan_fetch no image pointers; it reports the OR of the codes
 *   over all (ray, n), the rays that fail under any n, each once (more than RT_N_FAILED_MAX: the first of them in list
 *   order), and the counters of the one march.  There is no checking repeat: nothing is deposited.
 * fetch_length_spectra / length_spectra_ptrs: n = 2 .. N of the last run, anything else is RT_ERR_ARG; Iv [n_rays][K] (row
 *   stride K), ray2 [n_rays], err [n_rays], any pointer may be NULL.  On the device the rows of all lengths are one
 *   allocation, length-major (Iv [N-1][n_rays][K], ray2 and err [N-1][n_rays]); the pointers are valid until the next run or
 *   a change of the ray set.  The allocation is (N-1) n_rays K 8 bytes: a run that cannot have it fails with RT_ERR_NOMEM.
 * Not built: a chunked host-pointer loop like rt_hip_calc_rays, the multi-device arms, the C++ adapter, the one-launch form.
 *   (Several seed beams per length: rt_hip_plan_set_spectra_seeds, below; the ASE curve plus seeded curves of an emission plan:
 *   rt_hip_plan_set_length_spectra_ase_seeds, further below.) */
int rt_hip_plan_enable_length_spectra(rt_hip_plan *plan, int on);
int rt_hip_plan_fetch_length_spectra(rt_hip_plan *plan, int n, double *Iv, rt_ray *ray2, int32_t *err);
int rt_hip_plan_length_spectra_ptrs(rt_hip_plan *plan, int n, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev);

/* Spectra seeds: RayTrace::calc_ray under SEVERAL seed beams from one march -- the per-ray side of what rt_hip_plan_set_seeds,
 * _set_scan_seeds and _set_suffix_seeds do for the summed step records.  Neither the march record nor the boundary states hold
 * anything of the seed; it enters as Iv_s[k] = (f0_s f_s[4][k]) exp(gl[k]) only, so one march, one walk over the record and one
 * exponential per row serve every seed (rt_spec_seeds.hip in spectra mode, rt_spec_scan_seeds.hip in length spectra).
 * set_spectra_seeds installs seeds[0 .. n_seed), 1 <= n_seed <= RT_N_SEED_MAX, each validated as rt_hip_plan_create
 *   validates its seed, on a plan created WITH a seed (either method) whose spectra mode or length spectra are on.  The
 *   creation seed is not among them (pass it again if its rows are wanted); gain-only mode, method, scale and tables stay as
 *   created; on a forward ray grid the seeds' factor tables are built as for a set.  RT_ERR_ARG, each with its own text: a
 *   NULL plan, a plan created without a seed (an emission plan takes rt_hip_plan_set_spectra_ase_seeds), neither of
 *   the two modes on, more than RT_N_SEED_MAX seeds, invalid seeds; a rejected call leaves the installed seeds as they
 *   were.  n_seed = 0 removes the seeds and leaves the plain mode of the creation seed, bit for bit (these passes have no
 *   atomics on data).  rt_hip_plan_enable_spectra(0) and rt_hip_plan_enable_length_spectra(0) drop the seeds;
 *   rt_hip_plan_update_gain / _dev keep them.  While they are installed one of the two modes is on, so every switch and
 *   installer that refuses that mode refuses as before.
 * Outputs, seed-major in the one allocation of the mode: spectra mode Iv [n_seed][n_rays][K], err [n_seed][n_rays], ray2
 *   [n_rays]; length spectra Iv [n_seed][N-1][n_rays][K], err [n_seed][N-1][n_rays], ray2 [N-1][n_rays].  Error -1 and the exit
 *   ray do not depend on the seed.  Block 0 is seed 0: rt_hip_plan_fetch_spectra, _spectra_ptr, _fetch_length_spectra and
 *   _length_spectra_ptrs serve it unchanged.  A run that cannot have the allocation fails as the mode does (RT_ERR_NOMEM).
 *   Rows follow the single-seed modes: error -1 gives zeros and ray2 = 0 under every seed; a ray that fails -2 / -3 under
 *   seed s carries that code in err[s] only, -2 wins over -3; a row that is all zero on the CPU is all zero here.  Every
 *   Iv_s is the double the spectra (length-spectra) plan CREATED with seed s computes.
 * rt_hip_plan_fetch reports the OR of the codes over all (seed, ray, n), every failing ray once (more than RT_N_FAILED_MAX:
 *   the first of them in list order); err[s] holds seed s's codes ray by ray.  There is no checking repeat.
 * fetch_seed_spectra / seed_spectra_ptrs: s = 0 .. n_seed - 1 of the last spectra-mode run with seeds;
 * fetch_seed_length_spectra / seed_length_spectra_ptrs: likewise with n = 2 .. N of the last length-spectra run with seeds.
 *   Anything else is RT_ERR_ARG; any pointer may be NULL; device pointers are valid until the next run or a change of the
 *   ray set.
 * Not built: a chunked host-pointer loop, the multi-device arms, the C++ adapter, the one-launch form.
 *   (An emission plan -- the ASE spectrum plus seeded spectra: rt_hip_plan_set_spectra_ase_seeds, below.) */
int rt_hip_plan_set_spectra_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds);
int rt_hip_plan_fetch_seed_spectra(rt_hip_plan *plan, int s, double *Iv, rt_ray *ray2, int32_t *err);
int rt_hip_plan_seed_spectra_ptrs(rt_hip_plan *plan, int s, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev);
int rt_hip_plan_fetch_seed_length_spectra(rt_hip_plan *plan, int s, int n, double *Iv, rt_ray *ray2, int32_t *err);
int rt_hip_plan_seed_length_spectra_ptrs(rt_hip_plan *plan, int s, int n, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev);

/* Spectra mode with ASE seeds: RayTrace::calc_ray of an EMISSION problem and of the same problem under its seed beams from one
 * march -- the per-ray side of what rt_hip_plan_set_ase_seeds does for the summed step record.  Only evl depends on use_emis,
 * so the march record of an emission plan holds everything the gain-only pass of a seeded run of the same problem reads; one
 * march and one pass (rt_spec_ase_seeds.hip) leave 1 + n_seed blocks of rows per ray.
 * set_spectra_ase_seeds installs seeds[0 .. n_seed), 1 <= n_seed <= RT_N_SEED_MAX, each validated as rt_hip_plan_create
 *   validates its seed, on an emission plan (created without a seed, tables with E0, either method) whose spectra mode is on.
 *   There are no scales: calc_ray has none.  On a forward ray grid the seeds' factor tables are built as for a set.
 *   RT_ERR_ARG, each with its own text: a NULL plan, a plan created with a seed (it takes rt_hip_plan_set_spectra_seeds),
 *   tables without E0, spectra mode off, length spectra on (the text says "per-ray ASE seeds at every length are not built"; such
 *   a plan takes rt_hip_plan_set_length_spectra_ase_seeds, below, and this installer keeps its refusal), more than
 *   RT_N_SEED_MAX seeds, invalid seeds; a rejected call leaves the installed seeds as they were.  n_seed = 0 removes the seeds
 *   and leaves plain spectra mode, bit for bit (the pass has no atomics on data).  rt_hip_plan_enable_spectra(0) drops the
 *   seeds; rt_hip_plan_update_gain / _dev keep them.  While they are installed spectra mode is on, so every switch and
 *   installer that refuses that mode refuses as before.
 * Outputs, block-major in the one allocation of the mode: Iv [1 + n_seed][n_rays][K] (row stride K), err [1 + n_seed][n_rays],
 *   ray2 [n_rays].  Block 0 is the plan's own ASE spectrum -- the row the plan leaves without seeds, bit for bit, exact
 *   emission included --, so rt_hip_plan_fetch_spectra and _spectra_ptr serve it unchanged; block 1 + s is the row a
 *   spectra-mode plan leaves of the same problem created with seed s (E0 present, unused), bit for bit.  The allocation is
 *   (1 + n_seed) n_rays K 8 bytes: a run that cannot have it fails with RT_ERR_NOMEM.  Every element is written.  Error -1
 *   and the exit ray do not depend on the block: a -1 ray has zeros and -1 in every block; -2 / -3 are per block, -2 wins.
 *   A ray whose march sums are all zero has a row of zeros in block 0 and f0_s f_s[4][k] in block 1 + s.
 * rt_hip_plan_fetch reports the OR of the codes over all blocks, every failing ray once (more than RT_N_FAILED_MAX: the first
 *   of them in list order); err of block r holds its codes ray by ray.  There is no checking repeat.
 * fetch_full_spectra / full_spectra_ptrs: r = 0 (ASE) .. n_seed (1 + s: seed s) of the last such run.  Anything else is
 *   RT_ERR_ARG; any pointer may be NULL; device pointers are valid until the next run or a change of the ray set.
 * Not built: a chunked host-pointer loop, the multi-device arms, the C++ adapter, the one-launch form.
 *   (Length spectra with ASE seeds: rt_hip_plan_set_length_spectra_ase_seeds, below.) */
int rt_hip_plan_set_spectra_ase_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds);
int rt_hip_plan_fetch_full_spectra(rt_hip_plan *plan, int r, double *Iv, rt_ray *ray2, int32_t *err);   /* r = 0: ASE, 1 + s: seed s */
int rt_hip_plan_full_spectra_ptrs(rt_hip_plan *plan, int r, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev);

/* Length spectra with ASE seeds: RayTrace::calc_ray of an EMISSION problem and of the same problem under its seed beams at
 * EVERY plasma length n = 2 .. N, from ONE scan march and one pass (rt_spec_scan_ase_seeds.hip) -- the per-ray side of what
 * rt_hip_plan_set_scan_ase_seeds and _set_suffix_ase_seeds do for the summed step records, and what an emission length-spectra
 * plan plus a seeded length-spectra plan with rt_hip_plan_set_spectra_seeds leave from two marches.
 * set_length_spectra_ase_seeds installs seeds[0 .. n_seed), 1 <= n_seed <= RT_N_SEED_MAX, each validated as rt_hip_plan_create
 *   validates its seed, on an emission plan (created without a seed, tables with E0, either method) whose length spectra are
 *   on.  There are no scales: calc_ray has none.  The seeds' factor tables serve a forward ray grid only; the ray set of the
 *   run decides.  RT_ERR_ARG, each with its own text, in this order: a NULL plan, a plan created with a seed (it takes
 *   rt_hip_plan_set_spectra_seeds), tables without E0, spectra mode on (it takes rt_hip_plan_set_spectra_ase_seeds), length
 *   spectra off (rt_hip_plan_enable_length_spectra first), more than RT_N_SEED_MAX seeds, invalid seeds; a rejected call
 *   leaves the installed seeds as they were.  n_seed = 0 removes the seeds and leaves plain length spectra, bit for bit (the
 *   pass has no atomics on data).  rt_hip_plan_enable_length_spectra(0) drops the seeds; rt_hip_plan_update_gain / _dev keep
 *   them.  While they are installed length spectra are on, so every switch and installer that refuses that mode refuses as
 *   before.
 * A run does the scan march of the plan's method once, that march instance unchanged, and leaves, with L = N - 1, block-major
 *   then length-major in the one allocation of the mode: Iv [1 + n_seed][L][n_rays][K] (row stride K), err [1 + n_seed][L][n_rays],
 *   ray2 [L][n_rays]; block r L + n - 2 is curve r (0: ASE, 1 + s: seed s) at length n.  Block (0, n) is the row the plan leaves
 *   in plain length spectra, bit for bit, exact emission and its n = 3 rows included, so rt_hip_plan_fetch_length_spectra and
 *   _length_spectra_ptrs serve the ASE curve unchanged; block (1 + s, n) is the row a length-spectra plan leaves of the same
 *   problem created with seed s (E0 present, unused), bit for bit.  The state that serves length n is that of length spectra.
 *   Error -1 and ray2 do not depend on r: a -1 ray has zeros and -1 in every block of that n; -2 / -3 are per (r, n), -2 wins.
 *   A ray whose march sums are all zero has rows of zeros in the ASE curve and f0_s f_s[4][k] under seed s.  Every element is
 *   written; the allocation is (1 + n_seed) L n_rays K 8 bytes, and a run that cannot have it fails with RT_ERR_NOMEM.
 * rt_hip_plan_fetch reports the OR of the codes over all (r, ray, n), every failing ray once (more than RT_N_FAILED_MAX: the
 *   first of them in list order).  There is no checking repeat.
 * fetch_full_length_spectra / full_length_spectra_ptrs: r = 0 (ASE) .. n_seed (1 + s: seed s) and n = 2 .. N of the last such
 *   run.  Anything else is RT_ERR_ARG; any pointer may be NULL; device pointers are valid until the next run or a change of
 *   the ray set.
 * Not built: a chunked host-pointer loop, the multi-device arms, the C++ adapter, the one-launch form. */
int rt_hip_plan_set_length_spectra_ase_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds);
int rt_hip_plan_fetch_full_length_spectra(rt_hip_plan *plan, int r, int n, double *Iv, rt_ray *ray2, int32_t *err);   /* r = 0: ASE, 1 + s: seed s */
int rt_hip_plan_full_length_spectra_ptrs(rt_hip_plan *plan, int r, int n, double **Iv_dev, rt_ray **ray2_dev, int32_t **err_dev);

/* Host-pointer batched form of RayTrace::calc_ray: n independent calls in one.  rays and ray2 are [n][4] doubles
 * (x, y, a, b) as calc_ray takes and returns them; the coordinates are rounded to float exactly as calc_ray rounds
 * them (src/RayTraceImage.cpp:195-199).  Iv [n][K], err [n]; Iv, ray2, err and stats may be NULL.  gain: [N] tables
 * with Nv = K, seed may be NULL, method 1 (backward) or 2 (forward), dz the length of one plasma segment.  The rays are
 * traced in chunks whose spectra take at most 1 GiB of device memory, and a chunk travels to the host while the next
 * one runs, so device memory stays bounded for any n.  n = 0 is RT_OK; 2^32 - 4096 rays or more are RT_ERR_ARG.
 * stats: counters and kernel times summed over the chunks, total_ms = wall time of the call. */
int rt_hip_calc_rays(int device, int N, double dz, const rt_gain *gain, const rt_seed *seed, int K, int method,
                     const double *rays, size_t n, double *Iv, double *ray2, int32_t *err, rt_stats *stats);

/* Step mode: the arrays of the application's per-step record (intensity_step_struct, src/RayTraceStructures.h:361-369:
 * E_v, image, E_ang -- what sum_reduce sends and copy_step files) without the image cube.  With it enabled a run
 * produces, for the same rays, the reductions of what RayTraceImageCPULoop leaves in image[nx*ny*nv]
 * (RayTraceImageCPU.cpp:27-69: scale applied, only rays with both pixel indices >= 0 deposit, failing rays deposit nothing):
 *     E_v[k] = sum over pixels p of image[k + nv p]             k < nv, the frequency profile
 *     nf[p]  = sum over k of 2 dv[k] image[k + nv p]            p = ix + iy nx, the frequency-integrated near-field image
 *                                                               (the weight RayTraceImageCPU.cpp:66 gives I_ang)
 *     I_ang                                                     exactly as in image mode
 * and never allocates or writes an nx*ny*nv buffer.  The parent code's physical normalisation constants are not part of
 * the miniapp: they are linear factors, which the caller applies to these arrays.  W is not computed on this path.
 * The march runs as in image mode (two-kernel form; rt_hip_plan_last_fused is 0 -- unless the plan was told
 * otherwise, rt_hip_plan_set_step_one_launch below), rt_step_kernel
 * (raytrace-miniapp_amd/csrc/rt_step.hip) takes the place of the frequency kernel and computes every Iv of every ray as
 * that kernel does, bit for bit, rt_hip_plan_set_exact_emission included: rt_hip_plan_kernel_times and the timing ring
 * report it as freq_ms.  E_v is summed per work-group in LDS and added to the result once per work-group, nf with one
 * atomic per run of rays of a pixel (a plain store where the ray grid gives one ray per pixel): the sums differ from
 * those of the cube by summation order only.
 *   rt_hip_plan_run takes image_dev == NULL in this mode (anything else is RT_ERR_ARG) and an optional iang_dev;
 *   rt_hip_plan_fetch takes no image pointer (I_ang is served) and reports failure_code, failed rays and counters as
 *   ever; a run with error -2 / -3 is repeated in the checking mode, so the outputs are the reductions of what the CPU
 *   loop leaves.  E_v and nf belong to the plan (or are lent to it, set_step_buffers below) and are zeroed by every run.  Works with ray lists and ray grids (first /
 *   stride included), the probe, exact emission and debug bits 0 and 1; together with the path tracer or spectra mode
 *   it is RT_ERR_ARG.  A plan that has only run in step mode has no image buffer (rt_hip_plan_image_ptr == NULL);
 *   switching the mode off restores image mode unchanged.
 * fetch_step: waits for the last run (repeating a failing one) and copies out; any pointer may be NULL.  step_ptrs:
 * device pointers of E_v [nv] and nf [nx*ny] of the last run (for torch views / RCCL), valid while the plan lives.
 * rt_hip_step_loop is rt_hip_image_loop with E_v and nf in place of image: the same grid recognition, error convention
 * and staging of the (small) outputs behind the kernels.
 * set_step_buffers: E_v and nf in the caller's device memory, beside the caller's iang_dev -- so that the whole record is
 * one buffer a collective can take.  Every step run after the call zeroes E_v_dev [nv] and nf_dev [nx*ny] in its
 * zeroing launch and writes them in place of the plan's own arrays, the checking repeat of a failing run included;
 * fetch_step and step_ptrs serve whichever buffers the last run used.  NULL, NULL restores the plan's own allocation
 * (the default).  Alignment: 8 bytes each, what the kernels' f64 atomics and stores need (the plan's own nf sits at a
 * 256-byte boundary behind E_v; nothing requires it).  A misaligned pointer, or one pointer NULL and the other not, is
 * RT_ERR_ARG.  Outside step mode the call is accepted and takes effect when step mode is switched on.  The buffers must
 * stay valid until the last run that used them has been fetched.  One exception to the sizes: on a beam whose x or y
 * axis has a single grid point the reference's getIndex answers cell 1 for the coordinate g[0] + d/2 exactly
 * (RayTraceImageCPU.cpp:11-16, where the reference writes past its image); nf_dev then needs nx + 2 doubles more.
 *
 * rt_hip_multi_step_loop: rt_hip_step_loop on all devices of the node -- arguments and error convention of
 * rt_hip_step_loop with ndev in front; ndev, the communicator, the serialisation of callers and stats as in
 * rt_hip_multi_image_loop.  It is the application's multi-rank step (rays N_start + it N_parallel per rank,
 * src/RayTraceImage.cpp:300-313; ONE all-reduce of the record, intensity_step_struct::sum_reduce,
 * src/RayTraceStructures.cpp:1603-1646) inside one process: every device builds a plan on the FULL beam in step mode
 * and owns one buffer (E_v | pad to 256 bytes | nf | I_ang), lent to its plan through set_step_buffers and iang_dev.
 *   A list recognised as a tensor grid (the speculation and retry of rt_hip_multi_image_loop): device d generates rays
 *   d, d + ndev, ... (rt_hip_plan_set_ray_grid with first = d, stride = ndev); a device beyond the last ray contributes
 *   a record of zeros.  rt_hip_multi_last_mode reports 3.  Any other list: contiguous chunks of the list, mode 2.
 *   Never pixel-column tiles.
 *   Assembly: ONE ncclReduce(sum, f64) of the buffer -- nv + nx*ny + na*nb doubles and the pad -- to device 0, one
 *   download of the three arrays.  The image cube exists on no device and crosses no link.
 * A device with failing rays runs its checking repeat before its record travels: the sums are the reductions of what
 * RayTraceImageCPULoop leaves; failed rays are reported in the order of the devices (for a chunked list that is list
 * order: the report equals rt_hip_step_loop's).  The result differs from
 * rt_hip_step_loop's by summation order only.  RCCL with more than one rank has not run on hardware (as for the image
 * arm); RT_HIP_MULTI_LOOPBACK=n rehearses n workers on device 0 with the collective replaced by copies and a sum kernel. */
int rt_hip_plan_enable_step(rt_hip_plan *plan, int on);
int rt_hip_plan_set_step_buffers(rt_hip_plan *plan, double *E_v_dev, double *nf_dev);
int rt_hip_plan_fetch_step(rt_hip_plan *plan, double *E_v, double *nf, double *I_ang);
int rt_hip_plan_step_ptrs(rt_hip_plan *plan, double **E_v_dev, double **nf_dev);
int rt_hip_multi_step_loop(int ndev, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                           const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang,
                           unsigned int *failure_code, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats);
int rt_hip_step_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                     const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang,
                     unsigned int *failure_code, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats);

/* Step mode in ONE launch (opt-in; raytrace-miniapp_amd/csrc/rt_fused_step.hip): the march and the step pass as two phases
 * of the same persistent waves, what the one-launch run is for image mode.  on = 1: every following step run that can
 * takes it; on = 0 (the default, or RT_HIP_STEP_ONE_LAUNCH=1 in the environment at plan creation for on = 1): every step
 * run is the march kernel and rt_step_kernel.  Any other value is RT_ERR_ARG.  The call is accepted in any mode and takes
 * effect on step runs only; image, spectra and path runs are chosen as ever.
 *   Taken by: emission (no seed), backward method, on a ray grid of the beam (rt_hip_plan_set_ray_grid with the beam's own
 *   axes; first / stride / count included, any number of rays per pixel), march tables and step pass together within the
 *   LDS of a compute unit, an I_ang histogram of at most 32 KB.  Lent step buffers, the caller's iang_dev, exact emission
 *   and rt_hip_plan_update_gain work as in any step run.
 *   Keeps two kernels, silently: ray lists, seeded plans and seed sets, the probe, any debug bit, a grid with one ray per
 *   pixel on the beam's own image grid (the exclusive mode, whose nf is written by plain stores), tables that leave no
 *   room in LDS, RT_HIP_FUSED=2 in the environment, and the checking repeat of a failing run.
 * After a run that took it rt_hip_plan_last_fused is 1 and rt_hip_plan_kernel_times reports (launch, 0).  Every Iv of
 * every ray is the double rt_step_kernel computes; E_v, nf and I_ang differ from the two-kernel run's by summation order
 * only (the last tiles of a work-group are integrated in four parts of the frequency range, each adding its share). */
int rt_hip_plan_set_step_one_launch(rt_hip_plan *plan, int on);

/*
 * The gain tables of a resident plan replaced in place: a time loop whose plasma evolves has new n, g0, E0 and gv on the
 * same grids at every step, and keeps its plan -- ray grid, tangent and seed-factor tables, output mode, lent step
 * buffers, probe and timing ring included.  rt_gain_values holds the values of one length, in the shapes of the rt_gain
 * the plan was created with (gv: [cells][K], tight).  vals[0] is ignored as gain[0] is; N must equal the plan's; n, g0 and
 * gv must be non-NULL for lengths 1 .. N-1; E0 may be NULL and packs as zeros, as at creation.  use_emis, the grids, K,
 * the beam and the seed stay as created.
 *   Both calls first settle the plan's last run as rt_hip_plan_fetch does before it copies (wait, control block, the
 *   checking repeat of a run with error -2 / -3), so that a later fetch of that run serves ITS tables' result; device
 *   buffers of that run stay valid.
 *   Then: scan, validate, pack (raytrace-miniapp_amd/csrc/rt_tables.hip).  No run ever reads tables whose scan has not
 *   passed: an index of refraction that is not finite as the float the march rounds it to (a NaN, an infinity, a double
 *   beyond the largest float; rt_hip_plan_create refuses the same) -- on which the integrator would never advance -- a NULL pointer or a wrong N
 *   is RT_ERR_ARG and leaves every table of the plan untouched.  The scan recomputes, bit for bit, the four facts
 *   rt_hip_plan_create derives from the tables and every run is chosen by (rt_hip_plan_table_flags).
 *   update_gain_dev: device pointers, each checked to be device memory of the plan's device (anything else is
 *   RT_ERR_ARG).  The call enqueues on `stream`, waits once for the scan's summary, enqueues the pack and records an
 *   event, which the next rt_hip_plan_run waits for on whatever stream it runs.  The inputs follow stream semantics:
 *   unchanged until the work enqueued on `stream` has completed.
 *   update_gain: host pointers, free when the call returns: the raw values are uploaded into a scratch block and take
 *   the same device path.
 * table_flags: tables_bounded, ntest_proven (see rt_hip_plan_last_march_instance), whether a lineshape value is a NaN or
 * an infinity (emission mode), and gs_cap = 708 / max |gv|.  Any pointer may be NULL.
 */
typedef struct rt_gain_values {
    const double *n; /* [Nx*Ny] */
    const float *g0; /* [Nx*Ny] */
    const float *E0; /* [Nx*Ny], may be NULL */
    const float *gv; /* [Nx*Ny*Nv] */
} rt_gain_values;
int rt_hip_plan_update_gain(rt_hip_plan *plan, int N, const rt_gain_values *vals);
int rt_hip_plan_update_gain_dev(rt_hip_plan *plan, int N, const rt_gain_values *vals, void *stream);
int rt_hip_plan_table_flags(rt_hip_plan *plan, int *bounded, int *ntest_proven, int *gv_nonfinite, float *gs_cap);

/*
 * A seed set on a plan: the records of several seed beams from ONE march.  The application's per-step record
 * (intensity_step_struct, src/RayTraceStructures.h:361-369) holds one triple E_v_seed[s], image_seed[s], E_ang_seed[s] per
 * seed beam, s < N_seed <= N_SEED_MAX = RT_N_SEED_MAX.  The march does not depend on the seed (Helper.h:428-521); the seed
 * enters the frequency pass only, as Iv[k] = f0_s f_s[4][k] exp(gl[k]) (Helper.h:523-533, 569-580).  With a set installed
 * a step-mode run traces the rays once and leaves one record per seed (rt_step_seeds_kernel,
 * raytrace-miniapp_amd/csrc/rt_step_seeds.hip, in place of rt_step_kernel; reported as freq_ms): every Iv_s[k] is the
 * double a plan created with seed s computes, the sums differ from that plan's by summation order only.
 * set_seeds: the plan must have been created with a seed -- that decides the gain-only mode and the method, both stay as
 *   created; the creation seed is not part of the set (a caller who wants it passes it again).  n_seed = 1 ..
 *   RT_N_SEED_MAX installs seeds[0 .. n_seed), each validated as rt_hip_plan_create validates its seed (five complete
 *   tables, dim[4] == nv; dim[0 .. 3] are free); n_seed = 0 removes the set, the plan is then exactly as created.  The
 *   call first settles the plan's last run (as rt_hip_plan_update_gain does), copies the tables -- the caller's arrays are
 *   free when it returns -- and works before or after set_ray_grid / set_rays: on a forward ray grid every seed gets its
 *   own factor tables, rebuilt whenever the grid or the set changes.  A rejected call (RT_ERR_ARG) leaves the plan's set
 *   as it was.
 * With a set installed only step mode runs: rt_hip_plan_run outside step mode, with lent step buffers
 *   (rt_hip_plan_set_step_buffers) or with a non-NULL image_dev or iang_dev is RT_ERR_ARG, and so are
 *   rt_hip_plan_enable_path and rt_hip_plan_enable_spectra.  The probe, the timing ring, rt_hip_plan_kernel_times,
 *   rt_hip_plan_set_step_factor and rt_hip_plan_update_gain / _dev work as on any step plan; an update keeps the set.
 * Outputs: ONE allocation of the plan, n_seed blocks of equal stride, each
 *   (E_v[nv] | pad to 256 bytes | nf[nx*ny] (+ nx + 2 spare on a one-point x or y axis) | I_ang[na*nb] (+ na + 2 spare
 *   on a one-point a or b axis)) -- the layout of the buffer rt_hip_multi_step_loop builds per device -- the stride
 *   rounded up to 256 bytes, zeroed by the run's zeroing launch: a collective can take all records as one buffer.
 *   seed_step_ptrs: the device pointers of block s (any may be NULL), valid while the plan lives and the set stays.
 *   fetch_seed_step: waits for the run, runs the checking repeat where needed and copies block s; any pointer may be
 *   NULL; *failure_code is the code of seed s.  rt_hip_plan_fetch_step and rt_hip_plan_step_ptrs serve seed 0, and so
 *   does I_ang of rt_hip_plan_fetch.
 * Failures follow the reference run once per seed: error -1 does not depend on the seed -- the ray deposits into no
 *   record and every seed's code has the bit; error -2 / -3 under seed s removes the ray from record s only
 *   (RayTraceImageCPU.cpp:29-36, per create_image call).  rt_hip_plan_fetch reports the OR of the per-seed codes and the
 *   rays that fail under any seed, each once (more than RT_N_FAILED_MAX: the first of them in list order); the counters
 *   are those of one run, the rays being traced once.
 * Not taken with a set: image mode, spectra mode, the path tracer, the host-pointer and multi-device loops.
 */
int rt_hip_plan_set_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds);
int rt_hip_plan_fetch_seed_step(rt_hip_plan *plan, int s, double *E_v, double *nf, double *I_ang,
                                unsigned int *failure_code);
int rt_hip_plan_seed_step_ptrs(rt_hip_plan *plan, int s, double **E_v_dev, double **nf_dev, double **iang_dev);

/*
 * A length scan on a plan: the step record at EVERY plasma length n = 2 .. N from ONE forward march -- the gain-length
 * curve, which the application asks for with one create_image call per length (info->N = n, the first n tables).  With
 * the forward method RayTrace_calc_ray walks the lengths in order (Helper.h:430-441): its run with n lengths is the first
 * n - 1 iterations of its run with N.  Record n is, by definition, what a step run of the PREFIX problem leaves: the same
 * beam, rays, seed, scale and method with the tables gain[0 .. n); record N is the plain step record.
 *   The scan instance of the march (rt_march.hip, MARCH_OPT_SCAN) stores, beside the records, the state with which a ray
 *   crosses every length boundary; rt_step_scan_kernel (raytrace-miniapp_amd/csrc/rt_step_scan.hip, in place of
 *   rt_step_kernel; reported as freq_ms) places every ray once per length -- a ray that escapes inside length e counts as
 *   escaped for the lengths j >= e and as not escaped, with its boundary state, for j < e -- and deposits the running
 *   intensity whenever its walk over the sub-segments reaches a length.
 * enable_length_scan(on != 0): the plan's method must be 2 (forward), 3 <= N and N - 1 <= RT_N_SCAN_MAX, and it must hold
 *   no seed set; anything else is RT_ERR_ARG.  on = 0 restores the plan exactly as it was.  The call settles the plan's
 *   last run first.  With the scan on only step mode runs: rt_hip_plan_run outside step mode, with lent step buffers or
 *   with a non-NULL image_dev or iang_dev is RT_ERR_ARG, and so are rt_hip_plan_enable_path, rt_hip_plan_enable_spectra
 *   and rt_hip_plan_set_seeds with a non-empty set.  rt_hip_plan_set_step_one_launch is accepted, the run keeps two
 *   kernels.  Ray lists and ray grids (first / stride included), seeded and emission plans, exact emission, the probe, the
 *   timing ring, rt_hip_plan_set_step_factor and rt_hip_plan_update_gain / _dev work as on any step plan; an update keeps
 *   the scan on.
 * Outputs: ONE allocation of the plan, N - 1 blocks of the layout and stride of a seed set's (E_v | pad to 256 bytes | nf
 *   | I_ang, spares included), block n - 2 for n lengths, zeroed by the run's zeroing launch.  length_step_ptrs /
 *   fetch_length_step: n = 2 .. N as create_image counts lengths; any pointer may be NULL; *failure_code is the code of
 *   the run with n lengths.  rt_hip_plan_fetch_step, rt_hip_plan_step_ptrs and I_ang of rt_hip_plan_fetch serve record N.
 * Failures follow the reference run once per length: error -1 is s.z^2 < 0.01 of the state that serves the length and
 *   sets bit 1 in the codes of the lengths where it holds; error -2 / -3 at a length removes the ray from that length's
 *   record only.  rt_hip_plan_fetch reports the OR of the codes and the rays that fail at any length, each once (more than
 *   RT_N_FAILED_MAX: the first of them in list order); the counters are those of one run.
 * rt_hip_length_scan_loop: the host-pointer form, rt_hip_step_loop's arguments with one record per length: E_v
 *   [N-1][nv], nf [N-1][nx*ny], I_ang [N-1][na*nb], failure_codes [N-1], row n - 2 for n lengths (any may be NULL).
 * Not taken with the scan: the backward method (a run of n lengths starts in gain[n - 1]: no prefix), seed sets, the
 *   one-launch form, the multi-device loops, image, spectra and path runs.
 */
#define RT_N_SCAN_MAX 32 /* lengths of one scan: one mark bit per length and ray in the checking repeat */
int rt_hip_plan_enable_length_scan(rt_hip_plan *plan, int on);
int rt_hip_plan_fetch_length_step(rt_hip_plan *plan, int n, double *E_v, double *nf, double *I_ang, unsigned int *failure_code);
int rt_hip_plan_length_step_ptrs(rt_hip_plan *plan, int n, double **E_v_dev, double **nf_dev, double **iang_dev);
int rt_hip_length_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                            const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang,
                            unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats);

/*
 * A suffix scan on a plan: the step record of the run of the LAST n lengths, n = 2 .. N, from ONE backward march -- the
 * gain-length curve in the method RayTrace::create_image traces ASE with.  With the backward method RayTrace_calc_ray
 * starts at the launch ray and walks the lengths ii = N - 1, N - 2, ..., 1 (Helper.h:430-441): its first n - 1 outer
 * iterations are the whole run of the SUFFIX problem, an ordinary call with info->N = n and info->gain = gain + (N - n),
 * gain[0] kept in place 0 (gain[0].E0 decides the mode, nothing else of it is read).  Record n is, by definition, what a
 * step run of that problem leaves: the same beam, rays, seed, scale and method; record N is the plain step record.
 *   The march is the backward march with the boundary stores of the length scan (MARCH_OPT_SCAN: boundary m is the state
 *   after m marched segments).  rt_step_rscan_kernel (raytrace-miniapp_amd/csrc/rt_step_rscan.hip, in place of
 *   rt_step_kernel; reported as freq_ms) places the launch ray once -- the backward method deposits there, so pixel and
 *   angle cell are the same for every record -- and integrates the suffixes in chunks of four accumulators per walk over
 *   the sub-segments.  The state that serves record n (m = n - 1, e = the marched segment the ray escaped in): boundary m
 *   while m < e and m < N - 1, the ray not escaped; the final state otherwise.
 * enable_suffix_scan(on != 0): the plan's method must be 1 (backward), 3 <= N and N - 1 <= RT_N_SCAN_MAX, and it must hold
 *   no seed set, no ASE seeds and no length scan; anything else is RT_ERR_ARG.  on = 0 restores the plan exactly as it was.
 *   The call settles the plan's last run first.  Emission plans and seeded (gain-only) plans are taken.  With the scan on
 *   only step mode runs: rt_hip_plan_run outside step mode, with lent step buffers or with a non-NULL image_dev or
 *   iang_dev is RT_ERR_ARG, and so are rt_hip_plan_enable_path, rt_hip_plan_enable_spectra, rt_hip_plan_set_seeds with a
 *   non-empty set, rt_hip_plan_set_ase_seeds, rt_hip_plan_set_scan_seeds, rt_hip_plan_set_scan_ase_seeds and
 *   rt_hip_plan_enable_length_scan.  rt_hip_plan_set_step_one_launch is accepted, the run keeps two kernels.  Ray lists and
 *   ray grids (first / stride included), exact emission, the probe (exit ray, flags and steps of the whole run), the timing
 *   ring, rt_hip_plan_set_step_factor and rt_hip_plan_update_gain / _dev work as on any step plan; an update keeps the
 *   scan on.
 * Outputs: the length scan's -- N - 1 blocks of one allocation, block n - 2 for the last n lengths, served by
 *   rt_hip_plan_fetch_length_step and rt_hip_plan_length_step_ptrs; rt_hip_plan_fetch_step, rt_hip_plan_step_ptrs and
 *   I_ang of rt_hip_plan_fetch serve record N.  rt_hip_plan_history_append files the N - 1 records of such a run.
 * Failures follow the reference run once per record: error -1 is s.z^2 < 0.01 of the state that serves the record and
 *   sets bit 1 in the codes of the records where it holds; the seed factor of a seeded plan is taken at that state's
 *   position and exit angles and is 0 where the ray has escaped by then; error -2 / -3 under a record removes the ray from
 *   that record only.  rt_hip_plan_fetch reports the OR of the codes and the rays that fail anywhere, each once (more than
 *   RT_N_FAILED_MAX: the first of them in list order).
 * rt_hip_suffix_scan_loop: the host-pointer form, rt_hip_length_scan_loop's arguments; row n - 2 holds the record of the
 *   last n lengths.
 * Not taken with the suffix scan: the forward method, seed sets, the scan seeds of a length scan, the ASE seeds of a plain
 *   step or of a length scan (an emission plan takes rt_hip_plan_set_suffix_ase_seeds, a seeded plan
 *   rt_hip_plan_set_suffix_seeds, both below), the one-launch form, the multi-device loops, image, spectra and path runs.
 */
int rt_hip_plan_enable_suffix_scan(rt_hip_plan *plan, int on);
int rt_hip_suffix_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                            const rt_ray *rays, size_t n_rays, double scale, double *E_v, double *nf, double *I_ang,
                            unsigned int *failure_codes, rt_ray *failed_rays, int max_failed, int *n_failed, rt_stats *stats);

/*
 * The seeds of a scan: the step record of every seed beam at EVERY plasma length from ONE forward march.  The gain-length
 * curve is the observable of a seeded amplifier, and the application's step record holds one seeded triple per seed beam
 * (N_seed <= RT_N_SEED_MAX): neither the march nor the boundary states of the scan depend on the seed, which enters only as
 * Iv[k] = f0_s f_s[4][k] exp(gl[k]).  With scan seeds installed a step run of a scan plan leaves record (s, n) for
 * s < n_seed and n = 2 .. N: what a step run of the prefix problem of n lengths carrying seed s leaves -- record n of a plain
 * scan plan created with seed s, record s of a seed-set plan on the prefix problem.  rt_step_scan_seeds_kernel
 * (raytrace-miniapp_amd/csrc/rt_step_scan_seeds.hip, in place of rt_step_scan_kernel; reported as freq_ms) computes exp(gl)
 * of a length once for all seeds: every Iv_{s,n}[k] is the double the plain scan plan created with seed s computes, the sums
 * differ from that plan's by summation order only.
 * set_scan_seeds: accepted only while the length scan is on and on a plan created with a seed (which fixes the gain-only
 *   mode and the method and is not part of the set, as with rt_hip_plan_set_seeds); anything else is RT_ERR_ARG.  n_seed = 1
 *   .. RT_N_SEED_MAX installs seeds[0 .. n_seed), each validated as rt_hip_plan_set_seeds validates its seeds; n_seed = 0
 *   removes them, the plan is then a plain scan plan, bit for bit.  The call settles the plan's last run first, copies the
 *   tables and works before or after set_ray_grid / set_rays: on a forward ray grid every seed gets its own factor tables.
 *   A rejected call leaves the installed seeds as they were.  rt_hip_plan_enable_length_scan(plan, 0) drops them;
 *   rt_hip_plan_update_gain / _dev keep them.  The refusals of the scan and of the set stay as they are:
 *   rt_hip_plan_enable_length_scan still refuses a plan that holds a rt_hip_plan_set_seeds set, rt_hip_plan_set_seeds a
 *   non-empty set while the scan is on, and everything the scan refuses stays refused (lent step buffers, image_dev /
 *   iang_dev, path, spectra, the one-launch form, the multi-device loops).
 * Outputs: ONE allocation of the plan, zeroed by the run's zeroing launch: n_seed (N - 1) blocks of the seed-set layout and
 *   stride, record (s, n) = block s (N - 1) + (n - 2) -- a seed's curve is contiguous, a collective can take everything as
 *   one buffer.  seed_length_step_ptrs / fetch_seed_length_step: s < n_seed, n = 2 .. N (anything else is RT_ERR_ARG); any
 *   pointer may be NULL; *failure_code is the code of (s, n).  rt_hip_plan_fetch_length_step and
 *   rt_hip_plan_length_step_ptrs serve seed 0's curve; rt_hip_plan_fetch_step, rt_hip_plan_step_ptrs and I_ang of
 *   rt_hip_plan_fetch serve record (0, N).
 * Failures follow the reference run once per seed and length: error -1 depends on neither -- s.z^2 < 0.01 of the state that
 *   serves length j sets bit 1 in the code of (s, j) for every s; error -2 / -3 under seed s at length j removes the ray
 *   from record (s, j) only.  rt_hip_plan_fetch reports the OR of all codes and the rays that fail anywhere, each once (more
 *   than RT_N_FAILED_MAX: the first of them in list order); the counters are those of one run.  RT_N_SCAN_MAX stays 32: the
 *   checking repeat marks one bit per (seed, length) in a 64-bit word per ray.
 * rt_hip_seed_length_scan_loop: the host-pointer form, rt_hip_length_scan_loop's arguments with n_seed, seeds behind scale:
 *   E_v [n_seed][N-1][nv], nf [n_seed][N-1][nx*ny], I_ang [n_seed][N-1][na*nb], failure_codes [n_seed][N-1] (any may be
 *   NULL); n_seed = 1 .. RT_N_SEED_MAX.
 */
int rt_hip_plan_set_scan_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds);
int rt_hip_plan_fetch_seed_length_step(rt_hip_plan *plan, int s, int n, double *E_v, double *nf, double *I_ang,
                                       unsigned int *failure_code);
int rt_hip_plan_seed_length_step_ptrs(rt_hip_plan *plan, int s, int n, double **E_v_dev, double **nf_dev, double **iang_dev);
int rt_hip_seed_length_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                                 const rt_ray *rays, size_t n_rays, double scale, int n_seed, const rt_seed *seeds, double *E_v,
                                 double *nf, double *I_ang, unsigned int *failure_codes, rt_ray *failed_rays, int max_failed,
                                 int *n_failed, rt_stats *stats);

/*
 * ASE seeds on an emission plan: the WHOLE per-step record from ONE march.  intensity_step_struct is one buffer: the ASE
 * triple E_v | image | E_ang and one seeded triple per seed beam (N_seed <= RT_N_SEED_MAX).  The trajectory, gvl, ivl, the
 * exit state, the escape flag and the step count of RayTrace_calc_ray do not depend on use_emis, only evl does
 * (Helper.h:486-489, 502): the march of an emission plan leaves everything the gain-only pass of a seeded run reads.  With
 * ASE seeds installed a step-mode run marches once and rt_step_ase_seeds_kernel
 * (raytrace-miniapp_amd/csrc/rt_step_ase_seeds.hip, in place of rt_step_kernel; reported as freq_ms) leaves 1 + n_seed
 * records:
 *   record 0      the plan's own emission step record, what the plan leaves without the seeds;
 *   record 1 + s  what a step run leaves of the SAME PROBLEM CREATED WITH SEED s -- the same tables (E0 present but unused:
 *                 use_emis = E0 != NULL && seed == NULL), method and rays, scale scales[s]: gain-only,
 *                 Iv[k] = f0_s f_s[4][k] exp(gl[k]), the seed factor at the launch ray (method 2) or the exit ray (method 1).
 *   Every Iv is the double the plain emission plan, respectively the plain single-seed plan, computes; the sums differ from
 *   those plans' by summation order only.  The seeded records are sampled on the PLAN'S RAY SET, not on a separate
 *   seed-beam grid: the caller chooses one grid for all records (rt_hip_plan_set_ray_grid with its own axes, or a list).
 *   A ray whose march sums are all zero (counted in n_skipped) adds +0 to record 0 and is left out of it as ever, but it
 *   carries f0_s f_s[4][k] under a seed and is part of the seed records.
 * set_ase_seeds: accepted only on a plan created WITHOUT a seed whose tables carry E0 (an emission plan) and whose length
 *   scan is off; anything else is RT_ERR_ARG (rt_hip_plan_set_seeds keeps refusing such a plan).  n_seed = 1 ..
 *   RT_N_SEED_MAX installs seeds[0 .. n_seed), validated and copied as rt_hip_plan_set_seeds does it, factor tables per
 *   seed on a forward ray grid included (rebuilt when the grid or the seeds change); scales[s] is the scale of record
 *   1 + s, NULL: the plan's scale for all.  n_seed = 0 removes them, the plan is then a plain emission plan.  The call
 *   settles the plan's last run first; a rejected call changes nothing.
 * While installed only step mode runs: rt_hip_plan_run outside step mode, with lent step buffers or with a non-NULL
 *   image_dev or iang_dev is RT_ERR_ARG, and so are rt_hip_plan_enable_path, rt_hip_plan_enable_spectra and
 *   rt_hip_plan_enable_length_scan.  rt_hip_plan_set_step_one_launch is accepted, the run keeps two kernels.
 *   rt_hip_plan_update_gain / _dev (the seeds stay), exact emission, the probe, the timing ring and
 *   rt_hip_plan_set_step_factor work as on any step plan.
 * Outputs: ONE allocation of the plan, 1 + n_seed blocks of the seed-set layout and stride (E_v | pad | nf | I_ang), block 0
 *   ASE, block 1 + s seed s: a collective can take the application's whole buffer at once.  full_step_ptrs /
 *   fetch_full_step: r = 0 .. n_seed; any pointer may be NULL; *failure_code is the code of record r.
 *   rt_hip_plan_fetch_step, rt_hip_plan_step_ptrs and I_ang of rt_hip_plan_fetch serve block 0.
 * Failures follow the reference run once per record: error -1 puts the ray in no record and sets the bit in every
 *   record's code; error -2 / -3 under record r removes the ray from record r only.  rt_hip_plan_fetch reports the OR of
 *   the codes and the rays that fail under any record, each once (more than RT_N_FAILED_MAX: the first of them in list
 *   order); the counters are those of one run.
 * rt_hip_full_step_loop: the host-pointer form (a ray list): E_v [1+n_seed][nv], nf [1+n_seed][nx*ny], I_ang
 *   [1+n_seed][na*nb], failure_codes [1+n_seed] (may be NULL), row 0 ASE; n_seed = 1 .. RT_N_SEED_MAX.
 * Not taken: the multi-device loops, the one-launch form, a length scan, image, spectra and path runs.
 */
int rt_hip_plan_set_ase_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds, const double *scales);
int rt_hip_plan_fetch_full_step(rt_hip_plan *plan, int r, double *E_v, double *nf, double *I_ang, unsigned int *failure_code);
int rt_hip_plan_full_step_ptrs(rt_hip_plan *plan, int r, double **E_v_dev, double **nf_dev, double **iang_dev);
int rt_hip_full_step_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, int method, const rt_ray *rays,
                          size_t n_rays, double scale, int n_seed, const rt_seed *seeds, const double *scales, double *E_v,
                          double *nf, double *I_ang, unsigned int *failure_codes, rt_ray *failed_rays, int max_failed,
                          int *n_failed, rt_stats *stats);

/*
 * ASE seeds of a length scan: the WHOLE per-step record at EVERY plasma length from ONE forward march.  The two premises
 * are those of the two sections above: the march does not depend on the emission switch apart from evl, and the forward run
 * of n lengths is a prefix of the run of N.  With scan ASE seeds installed a step run of an emission scan plan marches once
 * (the scan march unchanged) and rt_step_scan_ase_seeds_kernel (raytrace-miniapp_amd/csrc/rt_step_scan_ase_seeds.hip, in
 * place of rt_step_scan_kernel; reported as freq_ms) leaves record (r, n) for r = 0 .. n_seed and n = 2 .. N:
 *   (0, n)      record n of the plain emission scan plan: what a step run of the prefix problem of n lengths leaves;
 *   (1 + s, n)  what a step run leaves of that prefix problem CREATED WITH SEED s -- the same tables, rays and method, scale
 *               scales[s]: gain-only, Iv[k] = f0_s f_s[4][k] exp(gl_n[k]), the seed factor at the launch ray, 0 where the
 *               ray has escaped by that length.
 *   Every Iv is the double the plain emission scan plan, respectively the scan plan created with a seed and holding seed s
 *   among its scan seeds, computes; the sums differ from those plans' by summation order only.  A ray whose march sums over
 *   the whole N-run are all zero (n_skipped) is left out of the ASE records and is part of the seed records.
 * set_scan_ase_seeds: accepted only on an emission plan (created without a seed, tables with E0) while its length scan is
 *   on; anything else is RT_ERR_ARG.  n_seed = 1 .. RT_N_SEED_MAX installs seeds[0 .. n_seed), validated and copied as
 *   rt_hip_plan_set_ase_seeds does it; scales[s] is the scale of the curve of seed s, NULL: the plan's scale for all.
 *   n_seed = 0 removes them: the plan is then a plain emission scan plan.  rt_hip_plan_enable_length_scan(plan, 0) drops
 *   them; rt_hip_plan_update_gain / _dev keep them; set_rays / set_ray_grid work before or after (the ray set of the run
 *   decides between the factor tables of a forward ray grid and the launch rays).  rt_hip_plan_set_step_one_launch is
 *   accepted, the run keeps two kernels.  The refusals of the neighbours stay: rt_hip_plan_set_ase_seeds refuses a scan
 *   plan, rt_hip_plan_enable_length_scan a plan with rt_hip_plan_set_ase_seeds seeds, rt_hip_plan_set_scan_seeds a plan
 *   created without a seed; everything the scan refuses stays refused (lent step buffers, image_dev / iang_dev, path,
 *   spectra).
 * Outputs: ONE allocation of the plan: (1 + n_seed) (N - 1) blocks of the seed-set layout and stride, record (r, n) = block
 *   r (N - 1) + (n - 2) -- a record's curve is contiguous, the ASE curve first.  full_length_step_ptrs /
 *   fetch_full_length_step: r = 0 .. n_seed, n = 2 .. N (anything else is RT_ERR_ARG); any pointer may be NULL;
 *   *failure_code is the code of (r, n).  rt_hip_plan_fetch_length_step and rt_hip_plan_length_step_ptrs serve the ASE
 *   curve; rt_hip_plan_fetch_step, rt_hip_plan_step_ptrs and I_ang of rt_hip_plan_fetch serve (0, N).
 *   rt_hip_plan_fetch_full_step and rt_hip_plan_fetch_seed_length_step are RT_ERR_ARG after such a run.
 *   (fetch_full_length_step and full_length_step_ptrs also serve the records of a suffix scan with ASE seeds, below.)
 * Failures follow the reference run once per (record, length): error -1 at length j puts the ray in no record of that
 *   length; error -2 / -3 under (r, j) removes the ray from (r, j) only.  rt_hip_plan_fetch reports the OR of all codes and
 *   the rays that fail anywhere, each once (more than RT_N_FAILED_MAX: the first of them in list order); the counters are
 *   those of one run.  RT_N_SCAN_MAX stays 32: the checking repeat marks one bit per (record, length) in 16 bytes per ray.
 * rt_hip_full_length_scan_loop: the host-pointer form, rt_hip_full_step_loop's arguments: E_v [1+n_seed][N-1][nv], nf
 *   [1+n_seed][N-1][nx*ny], I_ang [1+n_seed][N-1][na*nb], failure_codes [1+n_seed][N-1] (may be NULL).
 * Not taken: the multi-device loops, the one-launch form, image or spectra per length, the backward method.
 */
int rt_hip_plan_set_scan_ase_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds, const double *scales);
int rt_hip_plan_fetch_full_length_step(rt_hip_plan *plan, int r, int n, double *E_v, double *nf, double *I_ang,
                                       unsigned int *failure_code);
int rt_hip_plan_full_length_step_ptrs(rt_hip_plan *plan, int r, int n, double **E_v_dev, double **nf_dev, double **iang_dev);
int rt_hip_full_length_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, int method, const rt_ray *rays,
                                 size_t n_rays, double scale, int n_seed, const rt_seed *seeds, const double *scales,
                                 double *E_v, double *nf, double *I_ang, unsigned int *failure_codes, rt_ray *failed_rays,
                                 int max_failed, int *n_failed, rt_stats *stats);

/*
 * ASE seeds of a suffix scan: the WHOLE per-step record of the run of the LAST n lengths, n = 2 .. N, from ONE backward
 * march.  RayTrace::create_image traces ASE with the backward method, so the gain-length curve of an emission step is the
 * suffix scan above -- and the application's record of a step is the ASE triple plus one seeded triple per seed beam.  The
 * march does not depend on the emission switch apart from evl and not on a seed at all: with suffix ASE seeds installed a
 * step run of a backward emission plan whose suffix scan is on marches once (the suffix-scan march unchanged) and
 * rt_step_rscan_ase_seeds_kernel (raytrace-miniapp_amd/csrc/rt_step_rscan_ase_seeds.hip, in place of rt_step_rscan_kernel;
 * reported as freq_ms) leaves record (r, n) for r = 0 .. n_seed and n = 2 .. N:
 *   (0, n)      record n of the plain emission suffix-scan plan;
 *   (1 + s, n)  what a step run leaves of the suffix problem of the last n lengths CREATED WITH SEED s -- the same tables,
 *               rays and method, scale scales[s]: gain-only, Iv[k] = f0_{s,n} f_s[4][k] exp(gl_n[k]), the seed factor at the
 *               position and exit angles of the state that serves record n, 0 where the ray has escaped by then.
 *   Every Iv is the double the plain emission suffix-scan plan, respectively the suffix-scan plan created with seed s,
 *   computes; the sums differ from those plans' by summation order only.  A ray whose march sums over the whole N-run are
 *   all zero (n_skipped) is left out of the ASE records and is part of the seed records.
 * set_suffix_ase_seeds: accepted only on a backward (method 1) emission plan (created without a seed, tables with E0) while
 *   its suffix scan is on; a forward plan, a plan created with a seed, a plan whose suffix scan is off, more than
 *   RT_N_SEED_MAX seeds and a plan that holds ASE seeds, scan ASE seeds or a seed set are RT_ERR_ARG, each with its reason.
 *   n_seed = 1 .. RT_N_SEED_MAX installs seeds[0 .. n_seed), validated and copied as rt_hip_plan_set_ase_seeds does it;
 *   scales[s] is the scale of the curve of seed s, NULL: the plan's scale for all.  n_seed = 0 removes them: the plan is
 *   then a plain suffix-scan plan.  rt_hip_plan_enable_suffix_scan(plan, 0) drops them; rt_hip_plan_update_gain / _dev keep
 *   them.  Every refusal of the suffix scan stays: rt_hip_plan_set_seeds, rt_hip_plan_set_ase_seeds,
 *   rt_hip_plan_set_scan_seeds and rt_hip_plan_set_scan_ase_seeds refuse such a plan as before.
 * Outputs: the layout of a length scan with ASE seeds: (1 + n_seed) (N - 1) blocks of one allocation, record (r, n) = block
 *   r (N - 1) + (n - 2), served by rt_hip_plan_fetch_full_length_step and rt_hip_plan_full_length_step_ptrs;
 *   rt_hip_plan_fetch_length_step and rt_hip_plan_length_step_ptrs serve the ASE curve, rt_hip_plan_fetch_step,
 *   rt_hip_plan_step_ptrs and I_ang of rt_hip_plan_fetch record (0, N).  rt_hip_plan_history_append files all of them.
 * Failures follow the reference run once per (record, n): error -1 of the state that serves n puts the ray in no record
 *   (r, n) and sets bit 1 in each of their codes; error -2 / -3 under (r, n) removes the ray from (r, n) only; a failing ray
 *   is reported once.
 * rt_hip_full_suffix_scan_loop: the host-pointer form, the arguments and rows of rt_hip_full_length_scan_loop.
 * Not taken: the C++ adapter, the multi-device loops, the one-launch form (rt_hip_plan_set_step_one_launch is accepted, the
 *   run keeps two kernels).
 */
int rt_hip_plan_set_suffix_ase_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds, const double *scales);
int rt_hip_full_suffix_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, int method, const rt_ray *rays,
                                 size_t n_rays, double scale, int n_seed, const rt_seed *seeds, const double *scales,
                                 double *E_v, double *nf, double *I_ang, unsigned int *failure_codes, rt_ray *failed_rays,
                                 int max_failed, int *n_failed, rt_stats *stats);

/*
 * The seeds of a suffix scan: the step record of every seed beam of the run of the LAST n lengths, n = 2 .. N, from ONE
 * backward march -- what rt_hip_plan_set_scan_seeds is to the length scan, for a seeded amplifier traced with the backward
 * method.  Neither the march nor the boundary states depend on the seed: with suffix seeds installed a step run of a seeded
 * backward plan whose suffix scan is on marches once (the suffix-scan march of the seeded plan unchanged) and
 * rt_step_rscan_seeds_kernel (raytrace-miniapp_amd/csrc/rt_step_rscan_seeds.hip, in place of rt_step_rscan_kernel; reported
 * as freq_ms) leaves record (s, n) for s < n_seed and n = 2 .. N:
 *   (s, n)  what a step run leaves of the suffix problem of the last n lengths CREATED WITH SEED s -- the same tables, rays,
 *           method and scale: Iv[k] = f0_{s,n} f_s[4][k] exp(gl_n[k]), the seed factor at the position and exit angles of the
 *           state that serves record n, 0 where the ray has escaped by then.
 *   Every Iv is the double the suffix-scan plan created with seed s computes -- exp(gl_n) is taken once for all seeds --; the
 *   sums differ from that plan's by summation order only.
 * set_suffix_seeds: accepted only on a backward (method 1) plan created with a seed (which fixes the gain-only mode and is
 *   not part of the seeds, as with rt_hip_plan_set_scan_seeds) while its suffix scan is on; a forward plan, a plan created
 *   without a seed and a plan whose suffix scan is off are RT_ERR_ARG, each with its reason.  n_seed = 1 .. RT_N_SEED_MAX
 *   installs seeds[0 .. n_seed), validated and copied as rt_hip_plan_set_seeds does it (no factor tables: the backward
 *   method never takes the factor at a grid point); n_seed = 0 removes them: the plan is then a plain suffix-scan plan, bit
 *   for bit.  A rejected call leaves the installed seeds as they were.  rt_hip_plan_enable_suffix_scan(plan, 0) drops them;
 *   rt_hip_plan_update_gain / _dev keep them; rt_hip_plan_set_step_one_launch is accepted, the run keeps two kernels.  Every
 *   refusal of the suffix scan stays: rt_hip_plan_set_seeds, rt_hip_plan_set_ase_seeds, rt_hip_plan_set_scan_seeds,
 *   rt_hip_plan_set_scan_ase_seeds and rt_hip_plan_set_suffix_ase_seeds refuse such a plan as before.
 * Outputs: the layout of a length scan with scan seeds: n_seed (N - 1) blocks of one allocation, record (s, n) = block
 *   s (N - 1) + (n - 2), served by rt_hip_plan_fetch_seed_length_step and rt_hip_plan_seed_length_step_ptrs;
 *   rt_hip_plan_fetch_length_step and rt_hip_plan_length_step_ptrs serve seed 0's curve, rt_hip_plan_fetch_step,
 *   rt_hip_plan_step_ptrs and I_ang of rt_hip_plan_fetch record (0, N).  rt_hip_plan_history_append files all of them.
 * Failures follow the reference run once per (seed, n): error -1 of the state that serves n puts the ray in no record
 *   (s, n) and sets bit 1 in each of their codes; error -2 / -3 under (s, n) removes the ray from (s, n) only; a failing ray
 *   is reported once (more than RT_N_FAILED_MAX: the first of them in list order).  The checking repeat marks one bit per
 *   (seed, n) in a 64-bit word per ray.
 * rt_hip_seed_suffix_scan_loop: the host-pointer form, the arguments and rows of rt_hip_seed_length_scan_loop; method 1.
 * Not taken: the C++ adapter, the multi-device loops, the one-launch form.
 */
int rt_hip_plan_set_suffix_seeds(rt_hip_plan *plan, int n_seed, const rt_seed *seeds);
int rt_hip_seed_suffix_scan_loop(int device, int N, const rt_beam *beam, const rt_gain *gain, const rt_seed *seed, int method,
                                 const rt_ray *rays, size_t n_rays, double scale, int n_seed, const rt_seed *seeds, double *E_v,
                                 double *nf, double *I_ang, unsigned int *failure_codes, rt_ray *failed_rays, int max_failed,
                                 int *n_failed, rt_stats *stats);

/*
 * Step history: the step records of a time loop filed ON THE DEVICE.  What the application does on the host after every
 * step -- intensity_struct::copy_step (src/RayTraceStructures.cpp:1835-1867: E_v, image and E_ang of the ASE record and of
 * every seed record into slab i of arrays [N_t][...], E_sum[i] = sum_j image[j]), intensity_step_struct::valid() (:1647-1682)
 * and intensity_step_struct::add (:1579-1602) -- as ONE explicit call behind a step run, which only enqueues: two small
 * launches (raytrace-miniapp_amd/csrc/rt_history.hip) on the run's stream, no stream synchronise, no copy to the host, no
 * rt_hip_plan_fetch.  A step of  update_gain_dev -> run -> history_append  then has the one wait of the update left, and one
 * fetch at the end of the loop hands back the arrays.  Nothing happens unless these calls are made.
 * history_create: n_steps >= 1 sizes the history (an existing one is released first), n_steps = 0 releases it.  The memory
 *   is taken from the pool and zeroed at the FIRST append, which binds the history to the record set of that run (its kind,
 *   seeds and lengths: n_rec blocks, 1 after a plain step run) and to the beam sizes.
 * history_append: files the records of the last run -- which must have been a step run, anything else is RT_ERR_ARG -- into
 *   slab `step` (0 <= step < n_steps) of every array, for every block r of the run's record set at once:
 *     E_v[r][step][nv], nf[r][step][nx*ny], I_ang[r][step][na*nb]   bit-for-bit copies (of a plain step run: the buffers
 *                         rt_hip_plan_step_ptrs names, lent ones included, and the I_ang the run wrote, a caller's iang_dev
 *                         included); the spare cells behind nf / I_ang of a one-point beam axis are neither copied nor summed;
 *     E_sum[r][step]      sum of the nx*ny values of nf: a fixed partition of the pixels over work-groups, a fixed order
 *                         inside each, the partials added in index order by the second launch -- the same double from run to
 *                         run, whatever the slot, the block, the number of blocks or the place of the buffers (no atomics);
 *     flags[r][step]      bit 0: some value of E_v, nf or I_ang is < 0; bit 1: some value is NaN (valid() is flags == 0);
 *     code[r][step]       the failure code of block r, read on the device from the control block of the run;
 *     filled[step]        1.
 *   accumulate != 0 adds to the running sum as well: acc[r][.] = acc[r][.] + weight * x for every element of every block
 *   (the product rounded, then the sum: `acc + weight * x` of IEEE doubles without contraction) and E_sum_acc[r] likewise
 *   from E_sum[r][step].  weight is read only then.  stream NULL: the stream of the last run; another stream first waits for
 *   the run's end.  The records are filed AS THEY STAND in stream order: behind a bare rt_hip_plan_run a record with failing
 *   rays (code bits 2 / 3) is the unchecked one -- the reference gives the whole run up there ("Some rays failed") -- and a
 *   caller who wants the checked record calls any rt_hip_plan_fetch* first (the checking repeat) and appends then.  A slot
 *   appended twice holds the second record (the running sum took both).  A record set or beam sizes other than the ones the
 *   history is bound to are RT_ERR_ARG and leave the history as it was.  While an append is in flight the plan keeps an
 *   event behind it: a run on ANOTHER stream waits for it before it zeroes the records, and whatever frees or rewrites them
 *   from the host (destroy, a re-allocation, the checking repeat) waits for it; lent buffers are the caller's to keep.
 * history_ptrs / history_sum_ptrs: device pointers of block r (0 <= r < n_rec; after the first append): E_v [n_steps][nv], nf
 *   [n_steps][nx*ny], I_ang [n_steps][na*nb], E_sum [n_steps], code [n_steps], flags [n_steps]; of the running sum E_v [nv], nf
 *   [nx*ny], I_ang [na*nb], E_sum [1].  Any pointer may be NULL.  Read them on the append's stream or after a fetch.
 * history_fetch / history_fetch_sum: wait for the last append, then copy block r to the host (the same shapes; filled
 *   [n_steps]); any pointer may be NULL.  Before the first append everything reads zero (r = 0 only).
 * history_info: n_steps, n_rec (0 before the first append) and the number of slots an append was queued for.
 * rt_hip_debug_history_layout: the layout of the allocation and the shape of the two launches from plain numbers, by the
 *   function history_append itself uses; no device.  Both structs start with their own sizeof in `size`.  Offsets and strides
 *   in bytes: array X of block r and step i starts at off_X + r rec_X + i step_X (E_sum / code / flags: i * 8 / 4 / 4).
 *   chunk: pixels of nf per work-group (a constant); pix_wg work-groups per block sum nf, aux_wg take E_v and I_ang; grid =
 *   n_rec wg_per_rec work-groups of wg_threads; off_part / off_pflag: the scratch of the partials, [n_rec][wg_per_rec]
 *   doubles / words, scratch_bytes in all; the running sum (off_acc_*, rec_acc_*) is there when accumulate != 0 -- a plan's
 *   history always reserves it (one record per block beside n_steps of them).
 * Not taken: W, I_it (the reference files zero) and E_tot; histories of the multi-device loops; a host-pointer loop.
 */
typedef struct rt_hip_history_facts {
    unsigned size;
    int nv, nx, ny, na, nb, n_rec, n_steps, accumulate;
} rt_hip_history_facts;
typedef struct rt_hip_history_layout {
    unsigned size;
    unsigned chunk, wg_threads, pix_wg, aux_wg, wg_per_rec, grid;
    unsigned long long bytes, scratch_bytes;
    unsigned long long off_E_v, rec_E_v, step_E_v, off_nf, rec_nf, step_nf, off_I_ang, rec_I_ang, step_I_ang;
    unsigned long long off_E_sum, rec_E_sum, off_code, rec_code, off_flags, rec_flags, off_filled;
    unsigned long long off_acc_E_v, rec_acc_E_v, off_acc_nf, rec_acc_nf, off_acc_I_ang, rec_acc_I_ang, off_acc_E_sum;
    unsigned long long off_part, off_pflag;
} rt_hip_history_layout;
int rt_hip_plan_history_create(rt_hip_plan *plan, int n_steps);
int rt_hip_plan_history_append(rt_hip_plan *plan, int step, double weight, int accumulate, void *stream);
int rt_hip_plan_history_ptrs(rt_hip_plan *plan, int r, double **E_v, double **nf, double **I_ang, double **E_sum,
                             unsigned int **code, unsigned int **flags);
int rt_hip_plan_history_sum_ptrs(rt_hip_plan *plan, int r, double **E_v, double **nf, double **I_ang, double **E_sum);
int rt_hip_plan_history_fetch(rt_hip_plan *plan, int r, double *E_v, double *nf, double *I_ang, double *E_sum,
                              unsigned int *code, unsigned int *flags, unsigned char *filled);
int rt_hip_plan_history_fetch_sum(rt_hip_plan *plan, int r, double *E_v, double *nf, double *I_ang, double *E_sum);
int rt_hip_plan_history_info(rt_hip_plan *plan, int *n_steps, int *n_rec, int *n_filled);
int rt_hip_debug_history_layout(const rt_hip_history_facts *facts, rt_hip_history_layout *out);

/* Profiling aid (no reference counterpart): bit 0 = skip the frequency / deposit kernel, bit 1 = skip
 * the march and run the frequency pass over the records of the previous run of this plan, bit 2 = the
 * frequency kernel keeps its per-work-group I_ang sums to itself (I_ang stays zero).  0 = normal. */
int rt_hip_plan_set_debug(rt_hip_plan *plan, unsigned bits);

void rt_hip_plan_destroy(rt_hip_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
