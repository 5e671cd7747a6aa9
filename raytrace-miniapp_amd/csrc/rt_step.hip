#pragma once
// rt_step.hip -- step mode: the arrays of the application's per-step record (intensity_step_struct,
// src/RayTraceStructures.h:361-369) straight from the march records, without the image cube.
//
// What RayTraceImageCPULoop leaves in image[nx ny nv] (RayTraceImageCPU.cpp:27-69), reduced on the way:
//   E_v[k] = sum over pixels p of image[k + nv p]            the frequency profile
//   nf[p]  = sum over k of 2 dv[k] image[k + nv p]           the frequency-integrated near-field image
//   I_ang                                                     as the frequency kernel leaves it
// rt_step_kernel stands where rt_freq_kernel stands in the two-kernel run, reads the same tile-wise march records
// (rt_device.h) and has its shape: lanes = rays, a wave owns a tile of 64 consecutive rays, VEC frequencies per step,
// the float64 building blocks.  The per-ray preamble (rt_tile_ray.inc, then place_ray: seed factor, deposit cells,
// own-cell mode), the record decode with the tile-wide choice between ase_step_f32 / ase_step / ase_update
// (rt_tile_rec.inc) and the integration of a frequency batch (rt_tile_batch.inc) are the text that freq_tile includes
// -- so every Iv_r[k] is the value image mode computes for that ray, bit for bit, rt_hip_plan_set_exact_emission
// included.  Only the early-out rule and the deposit are step_tile's own:
//   E_v   : per batch of VEC frequencies one sum over the lanes that deposit into the image (pixel valid, ray live),
//           the wave sum rt_step_evsum.inc, times scale, added to the work-group's E_v[Kp] in LDS; flushed once per
//           work-group at the end of the launch with f64 atomics, like the I_ang histogram.  No global atomic per ray
//           and frequency.
//   nf    : the lane's sum over k of 2 dv[k] Iv[k] (the I_ang value) times scale, reduced over runs of lanes with
//           equal pixel by one segmented scan per tile (rt_wave_runs.inc, rt_wave_runscan.inc), one f64 global atomic
//           per run -- a plain store where the host has proved one ray per pixel (DevParams::exclusive).
// Nothing of nx ny nv is allocated or written.  Failing runs take the checking repeat of the frequency kernel
// (plan_repeat_checked): FQ_SAFE_CHECK integrates without depositing and marks, FQ_SAFE_SKIP leaves the marked rays out.
// The body of step_tile is a text fragment, rt_tile_step.inc: the one-launch run (rt_fused_step.hip) includes the same text
// for a part of a tile's frequency range.  The shell of the kernel is text as well, shared with the step passes of a seed
// set (rt_step_seeds.hip) and of a length scan (rt_step_scan.hip): the work-group's LDS, its prologue and its epilogue
// (rt_step_wg.inc) and the tile hand-out (rt_step_handout.inc).
#include "rt_spec.hip" // (and rt_freq.hip through it)
#include "rt_step.h"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip)

// the LDS of a work-group of a step pass: the strides of its histograms and its size (rt_step_wg.inc, beside the carving)
#define STEP_WG_SIZE
#include "rt_step_wg.inc"
#undef STEP_WG_SIZE

template <int SF, bool EMIS>
__device__ __forceinline__ void step_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, double *lds_iang,
                                          double *lds_ev, const double *tab, double *xpose, const unsigned tile, const int lane)
{
    // (a whole tile: all K frequencies, error -1 reported here)
#define TILE_K0 0
#define TILE_K_END K
#define TILE_REPORTS_ERR1 true
#include "rt_tile_step.inc"
#undef TILE_K0
#undef TILE_K_END
#undef TILE_REPORTS_ERR1
}

// One work-group of FREQ_WG_WAVES waves per CU: the shell every step pass has -- prologue (rt_step_wg.inc: the LDS of one
// record, pass_shape sizes it with step_lds_doubles), tile hand-out (rt_step_handout.inc: the tiles rt_freq_kernel hands
// out, by its rule, guided chunks for the gain-only instance), epilogue (rt_step_wg.inc).
template <int SF, bool EMIS>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_step_kernel(const StepKArg A)
{
    const FreqHot &H = A.hot;
#define STEP_WG_NREC 1
#define STEP_WG_ANG_STRIDE step_ang_stride(n_ang)
#define STEP_WG_ANG_ZERO n_ang
#define STEP_WG_ONE_RECORD
#define STEP_WG_RECORD(r)
#define STEP_WG_EV(r, c) A.out.E_v[c]
#define STEP_WG_IANG(r, c) H.iang[c]
#define STEP_WG_PROLOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_PROLOGUE
    const int lane = lane_id();
    // the cold half of the argument block, the flag word and the lane number opaque per tile, as in rt_freq_kernel
#define HANDOUT_TILES_PER_FETCH (EMIS ? FREQ_TILES_PER_FETCH_EMIS : FREQ_TILES_PER_FETCH_GAIN)
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(StepKArg, cold));            \
    asm volatile("" : "+s"(C));                                                                                                        \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    asm volatile("" : "+s"(hflags), "+v"(lane_t));                                                                                     \
    step_tile<SF, EMIS>(H, hflags, C, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
#include "rt_step_handout.inc"
#undef HANDOUT_TILES_PER_FETCH
#undef HANDOUT_TILE
#define STEP_WG_EPILOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_EPILOGUE
#undef STEP_WG_NREC
#undef STEP_WG_ANG_STRIDE
#undef STEP_WG_ANG_ZERO
#undef STEP_WG_ONE_RECORD
#undef STEP_WG_RECORD
#undef STEP_WG_EV
#undef STEP_WG_IANG
}

} // namespace rt
