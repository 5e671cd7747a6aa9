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
//           the wave sum of the few-runs deposit of rt_freq.hip, times scale, added to the work-group's E_v[Kp] in LDS;
//           flushed once per work-group at the end of the launch with f64 atomics, like the I_ang histogram.  No
//           global atomic per ray and frequency.
//   nf    : the lane's sum over k of 2 dv[k] Iv[k] (the I_ang value) times scale, reduced over runs of lanes with
//           equal pixel by one segmented scan per tile, one f64 global atomic per run -- a plain store where the host
//           has proved one ray per pixel (DevParams::exclusive).
// Nothing of nx ny nv is allocated or written.  Failing runs take the checking repeat of the frequency kernel
// (plan_repeat_checked): FQ_SAFE_CHECK integrates without depositing and marks, FQ_SAFE_SKIP leaves the marked rays out.
// The body of step_tile is a text fragment, rt_tile_step.inc: the one-launch run (rt_fused_step.hip) includes the same text
// for a part of a tile's frequency range.
#include "rt_spec.hip" // (and rt_freq.hip through it)
#include "rt_step.h"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip)

// doubles of dynamic LDS of a work-group (layout: rt_step_kernel)
inline size_t step_lds_doubles(bool iang_in_lds, int n_ang, int Kp, int wg_waves)
{
    return (size_t) 2 * EXP_TAB + (iang_in_lds ? (size_t) ((n_ang + 1) & ~1) : 0) + (size_t) Kp + (size_t) wg_waves * (size_t) (4 * XP_ROW);
}

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

// One work-group of FREQ_WG_WAVES waves per CU, tiles handed out from the eight sharded counters of the control block
// exactly as rt_freq_kernel hands them out (DevCtl::next_tile_f, guided chunks for the gain-only instance).
// LDS of a work-group, all dynamic (launch_step sizes it with step_lds_doubles):
//   [the two exponent tables of rt_freq_kernel][I_ang histogram, na*nb doubles rounded up to even (if it fits)]
//   [E_v accumulator, Kp doubles][per wave: the transposition rows [4][XP_ROW] of the wave sum]
template <int SF, bool EMIS>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_step_kernel(const StepKArg A)
{
    extern __shared__ __align__(16) unsigned char step_lds[];
    const FreqHot &H       = A.hot;
    const bool iang_in_lds = (H.flags & FQ_IANG_LDS) != 0;
    const int n_ang        = H.n_ang;
    double *exp2_tab       = reinterpret_cast<double *>(step_lds);
    double *lds_iang       = iang_in_lds ? exp2_tab + 2 * EXP_TAB : nullptr;
    double *lds_ev         = exp2_tab + 2 * EXP_TAB + (iang_in_lds ? ((n_ang + 1) & ~1) : 0);
    double *xpose          = lds_ev + H.Kp + (size_t) (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)) * (size_t) (4 * XP_ROW);
    RT_FILL_EXP_TABLES(exp2_tab)
    if (lds_iang) {
        for (int c = (int) threadIdx.x; c < n_ang; c += (int) blockDim.x)
            lds_iang[c] = 0.0;
    }
    for (int c = (int) threadIdx.x; c < H.Kp; c += (int) blockDim.x)
        lds_ev[c] = 0.0;
    __syncthreads();
    const int lane             = lane_id();
    const unsigned n_tiles_run = H.tile_end - H.tile_begin;
    unsigned shard = blockIdx.x & 7u, tried = 0;
    auto shard_size = [&](unsigned sh) { return (n_tiles_run + 7u - sh) / 8u; };
    unsigned s_n    = shard_size(shard);
    const unsigned sh_shift = H.fetch_shift > 3 ? H.fetch_shift - 3 : 0;
    constexpr unsigned TILES_PER_FETCH = EMIS ? FREQ_TILES_PER_FETCH_EMIS : FREQ_TILES_PER_FETCH_GAIN;
    auto chunk_of = [&](unsigned left) {
        const unsigned c = left >> sh_shift;
        return c < 1u ? 1u : (c > TILES_PER_FETCH ? TILES_PER_FETCH : c);
    };
    unsigned tch = chunk_of(s_n);
    // (the reservation and the walk over its tiles as two nested loops: as rt_freq_kernel's single loop with a window of
    // reserved tiles the gain-only instance kept 48 bytes of stack for its loop state)
    for (;;) {
        unsigned base = 0;
        if (lane == 0)
            base = atomicAdd(&H.ctl->next_tile_f[H.freq_id][shard][0], tch);
        base = (unsigned) __builtin_amdgcn_readfirstlane((int) base);
        if (base >= s_n) { // this shard is empty: on to the next one, until all eight have been seen empty
            if (++tried == 8)
                break;
            shard = (shard + 1) & 7u;
            s_n   = shard_size(shard);
            tch   = 1; // a guest takes single tiles
            continue;
        }
        const unsigned t_end = s_n - base < tch ? s_n : base + tch;
        tch                  = chunk_of(s_n - t_end);
        for (unsigned t = base; t < t_end; t++) {
            const unsigned tile = H.tile_begin + t * 8u + shard;
            // the cold half of the argument block, the flag word and the lane number opaque per tile, as in rt_freq_kernel
            ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(StepKArg, cold));
            asm volatile("" : "+s"(C));
            unsigned hflags = H.flags;
            int lane_t      = lane;
            asm volatile("" : "+s"(hflags), "+v"(lane_t));
            step_tile<SF, EMIS>(H, hflags, C, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
        }
    }
    // the work-group's sums leave once: coalesced native f64 atomics (zeros, most of a small launch's histogram, stay)
    __syncthreads();
    for (int c = (int) threadIdx.x; c < H.K; c += (int) blockDim.x) {
        const double v = lds_ev[c];
        if (v != 0.0)
            unsafeAtomicAdd(&A.out.E_v[c], v);
    }
    if (lds_iang && !(H.flags & FQ_DBG_NOFLUSH)) {
        for (int c = (int) threadIdx.x; c < n_ang; c += (int) blockDim.x) {
            const double v = lds_iang[c];
            if (v != 0.0)
                unsafeAtomicAdd(&H.iang[c], v);
        }
    }
}

} // namespace rt
