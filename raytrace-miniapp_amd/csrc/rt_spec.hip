#pragma once
// rt_spec.hip -- spectra mode: RayTrace::calc_ray (src/RayTraceImage.cpp:189-204) for every ray of a run.
//
// What RayTrace_calc_ray does after the march (Helper.h:514-594), per ray and with nothing deposited: the -1 test, the
// exit ray, the seed spectrum of a seeded, non-escaped ray, the emission recurrence per sub-segment or the gain-only
// product, then the -2 / -3 scan.  Reads the tile-wise march records (rt_device.h) as rt_freq_kernel does and has its
// shape: lanes = rays, a wave owns a tile of 64 consecutive rays, VEC frequencies per step, the float64 building
// blocks of rt_freq.hip.  The loads of the preamble and the failure report (rt_tile_ray.inc), the record decode with the
// tile-wide choice of the update (rt_tile_rec.inc) and the integration of a frequency batch (rt_tile_batch.inc) are the
// text that freq_tile includes, so the two modes take the same arithmetic, rt_hip_plan_set_exact_emission included;
// spectra mode's own are the exit ray, its early-out rule (a tile without a live ray still writes its rows of zeros), the
// staging and the stores, and the -2 / -3 scan: rt_spec_tile.inc, the text that spec_tile shares with the passes that carry
// seeds (rt_spec_seeds.hip, rt_spec_ase_seeds.hip).
//
// Outputs: Iv [n_rays][K] (row stride K, not Kp), ray2 [n_rays], err [n_rays].  No image, no I_ang, no atomics on data.
//
// The stores are the hot part: n K 8 bytes, more than the image path moves.  A lane that wrote its own row would
// put the 64 lanes of a store instruction into 64 rows; instead the wave stages 16 frequencies of its 64 rows in LDS
// ([64][XS_ROW], the staging of the exclusive deposit in rt_freq.hip) and writes them as row segments of 128
// contiguous bytes, 16 bytes per lane and eight rows per instruction.  A tile's output is one contiguous block of
// 64 K doubles, so the eight row segments of an instruction lie K doubles apart inside it.
#include "rt_freq.hip"
#include "rt_spec.h"

namespace rt {

// the LDS of a work-group of a per-ray spectra pass: its size (rt_spec_wg.inc, beside the carving)
#define SPEC_WG_SIZE
#include "rt_spec_wg.inc"
#undef SPEC_WG_SIZE

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip; the float32 preamble has nothing to contract)

// 16 bytes from the staging rows to the output: written once, never read by this kernel
// Ordinary stores: the 128-byte row segments of a group start wherever the row does (K doubles apart: 32 bytes off a
// cache line per row for K = 52, 16 for K = 82), so most segments cover two lines in part and the next group of the same
// row fills them up a few microseconds later -- in L2, if the lines may stay there.  The streaming stores of the exclusive
// deposit (whole aligned lines there) send the parts to memory one by one: measured 1.89 against 1.27 ms on the stand-in,
// 4.20 against 2.42 ms on seed_small (profiles/spectra_ab.txt).
typedef double f64x2s __attribute__((ext_vector_type(2)));
#define SPEC_STORE16(src, dst) (*reinterpret_cast<f64x2s *>(dst) = *reinterpret_cast<const f64x2s *>(src))

template <int SF, bool EMIS>
__device__ __forceinline__ void spec_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, const SpecOut &O, const double *tab,
                                          double *stage, const unsigned tile, const int lane)
{
    const bool seeded = (hflags & FQ_HAS_SEED) != 0;

    double f0         = 0.0;

    // ---- the tile head (rt_spec_tile.inc): record, -1 test, exit ray, probe; the seed factor (Helper.h:523-533) ----
    // the seed factor of place_ray (rt_freq.hip), the image path's own: asked for the exit angles and for own-cell
    // placement, which is two index computations that nothing here uses -- no grid is searched, none is needed
#define SPEC_TILE_HEAD
#define SPEC_TILE_NEED_RAY (seeded && !backward) // the forward seed is taken at the launch ray
#define SPEC_TILE_RAY2 O.ray2
#define SPEC_TILE_AT_EXIT                                                                                       \
    if (seeded && !(fl & F_ESCAPED))                                                                            \
        f0 = place_ray(FQ_HAS_SEED | FQ_NEED_EXIT | FQ_OWN_CELLS, C, R, 0, backward, ridx, m, fl, ray).f0;
#include "rt_spec_tile.inc"
#undef SPEC_TILE_AT_EXIT
#undef SPEC_TILE_RAY2
#undef SPEC_TILE_NEED_RAY
#undef SPEC_TILE_HEAD
    // a ray with error -1, and one whose every update is the identity (F_SKIP), gets a row of zeros
    const bool live     = have && !err1 && !(fl & F_SKIP);
    const bool any_live = __ballot(live) != 0ull;

    // ---- the march record of this lane's ray, the slots of a lane without a live ray zeroed ----
#define TILE_MASK live
#include "rt_tile_rec.inc"
#undef TILE_MASK
    const ConstF64 sfk = (ConstF64) (unsigned long long) H.seed_fk;
    // a full tile and an even K: every 16-frequency group that lies inside K leaves as 16-byte stores
    const bool wide_ok = row0 + WAVE <= n_rays && (K & 1) == 0;

    // ---- the frequencies: integration, scan, staging and stores (rt_spec_tile.inc) ----
#define SPEC_TILE_EMISSION
#define SPEC_TILE_IV O.Iv
#include "rt_spec_tile.inc"
#undef SPEC_TILE_IV
#undef SPEC_TILE_EMISSION
    const bool bad_neg = live && iv_min < 0.0, bad_nan = live && has_nan;
    if (have)
        O.err[ridx] = err1 ? -1 : (bad_neg ? -2 : (bad_nan ? -3 : 0));
    if (bad_neg || bad_nan)
        report_failure(bad_neg ? (1u << 2) : (1u << 3));
}

// One work-group of FREQ_WG_WAVES waves per CU, tiles handed out from the eight sharded counters of the control block
// (DevCtl::next_tile_f, rt_freq_kernel says why eight), one tile per fetch: every tile costs the same here.
// LDS of a work-group, all dynamic: the two exponent tables of rt_freq_kernel, then [64][XS_ROW] staging doubles per wave.
template <int SF, bool EMIS>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_spec_kernel(const SpecKArg A)
{
#define SPEC_WG_KERNEL
#define SPEC_WG_KARG SpecKArg
#define SPEC_WG_CALL spec_tile<SF, EMIS>(H, hflags, C, A.out, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_CALL
#undef SPEC_WG_KARG
#undef SPEC_WG_KERNEL
}

} // namespace rt
