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
// spec_tile's own are the exit ray, its early-out rule (a tile without a live ray still writes its rows of zeros), the
// staging and the stores, and the -2 / -3 scan.
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
    const int S           = SF ? SF : H.L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned row0   = tile * WAVE;
    const unsigned ridx   = row0 + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = H.method == 1;
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;
    const bool seeded     = (hflags & FQ_HAS_SEED) != 0;

    // ---- per-ray preamble: record, -1 test, exit ray, seed factor (Helper.h:514-533) ----
#define TILE_NEED_RAY (seeded && !backward) // the forward seed is taken at the launch ray
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    rt_ray r2       = { 0.0f, 0.0f, 0.0f, 0.0f };            // (the reference leaves ray2 untouched on error -1: zeros here)
    double f0       = 0.0;
    if (have && !err1) {
        r2.x = m.px; // Helper.h:518-521
        r2.y = m.py;
        r2.a = atanf_flt32_kernel(m.sx / m.sz) * 1e3f;
        r2.b = atanf_flt32_kernel(m.sy / m.sz) * 1e3f;
        // the seed factor of place_ray (rt_freq.hip), the image path's own: asked for the exit angles and for own-cell
        // placement, which is two index computations that nothing here uses -- no grid is searched, none is needed
        if (seeded && !(fl & F_ESCAPED))
            f0 = place_ray(FQ_HAS_SEED | FQ_NEED_EXIT | FQ_OWN_CELLS, C, R, 0, backward, ridx, m, fl, ray).f0;
    }
    if (have) {
        O.ray2[ridx] = r2;
        if (probe_on) {
            C->probe.ray2[ridx]  = r2;
            C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
            C->probe.steps[ridx] = steps;
        }
    }
    if (err1)
        report_failure(1u << 1);
    // a ray with error -1, and one whose every update is the identity (F_SKIP), gets a row of zeros
    const bool live     = have && !err1 && !(fl & F_SKIP);
    const bool any_live = __ballot(live) != 0ull;

    // ---- the march record of this lane's ray, the slots of a lane without a live ray zeroed ----
#define TILE_MASK live
#include "rt_tile_rec.inc"
#undef TILE_MASK
    const ConstF64 sfk = (ConstF64) (unsigned long long) H.seed_fk;

    double iv_min = 0.0;   // min over k of Iv, NaNs ignored: negative <=> error -2
    bool has_nan  = false; // error -3 unless -2 (Helper.h:588-593: negative wins)
    // a full tile and an even K: every 16-frequency group that lies inside K leaves as 16-byte stores
    const bool wide_ok = row0 + WAVE <= n_rays && (K & 1) == 0;

    for (int kb = 0; kb < K; kb += VEC) {
        double Iv[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            Iv[j] = 0.0;
        if (any_live) { // (else nothing to integrate: the rows are zeros)
#define TILE_READ_SLOT rec_slot_lazy
#define TILE_REREAD live
#include "rt_tile_batch.inc"
#undef TILE_READ_SLOT
#undef TILE_REREAD
        }
        // ---- scan (Helper.h:582-587) and staging: the lane's four values into its staging row ----
        double *mine = stage + lane * XS_ROW + (kb & 12);
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const double v = (live && kb + j < K) ? Iv[j] : 0.0; // (the padding columns K .. Kp-1 are not part of the spectrum)
            iv_min         = fmin(iv_min, v);
            has_nan        = has_nan || v != v;
            mine[j]        = v;
        }
        if ((kb & 12) == 12 || kb + VEC >= K) {
            __builtin_amdgcn_wave_barrier();
            const int kbase = kb & ~15;
            const int width = K - kbase < 16 ? K - kbase : 16; // frequencies of this group
            if (wide_ok && width == 16) {
                // eight lanes cover the 128 staged bytes of a row, a store instruction eight rows
                double *dst        = O.Iv + ((size_t) (row0 + (unsigned) (lane >> 3)) * (size_t) K + (size_t) (kbase + 2 * (lane & 7)));
                const size_t gstep = (size_t) 8 * (size_t) K; // eight rows on
                const double *src  = stage + (lane >> 3) * XS_ROW + 2 * (lane & 7);
#pragma unroll 4
                for (int g = 0; g < WAVE / 8; g++)
                    SPEC_STORE16(src + g * 8 * XS_ROW, dst + (size_t) g * gstep);
            } else if (wide_ok) {
                // the last, narrower group of a row (2 .. 14 frequencies): still 16 bytes per lane, the wave's lanes dealt over
                // the 64 x hw pieces row by row.  (Folding a left-over of two frequencies into the group before it, as rows
                // of 18 in the two spare doubles of the staging rows, was built and measured: seed_small, K = 82, 2.375
                // against 2.413 ms, the stand-in, which has no such left-over, 1.254 against 1.226 ms.  Not kept.)
                const unsigned hw = (unsigned) width >> 1; // 16-byte pieces per row
                for (unsigned q = (unsigned) lane; q < WAVE * hw; q += WAVE) {
                    const unsigned row = q / hw, piece = q - row * hw;
                    SPEC_STORE16(stage + row * XS_ROW + 2 * piece, O.Iv + ((size_t) (row0 + row) * (size_t) K + (size_t) kbase + 2 * piece));
                }
            } else {
                // ragged tile or odd K: 8 bytes per lane, four rows per instruction
                const int k = kbase + (lane & 15);
#pragma unroll 4
                for (int g = 0; g < WAVE / 4; g++) {
                    const unsigned row = row0 + (unsigned) (4 * g + (lane >> 4));
                    if (row < n_rays && k < K)
                        O.Iv[(size_t) row * (size_t) K + (size_t) k] = stage[(4 * g + (lane >> 4)) * XS_ROW + (lane & 15)];
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
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
    // per tile: the cold half of the argument block, the flag word and the lane number opaque, as in rt_freq_kernel
#define SPEC_WG_KERNEL
#define SPEC_WG_TILE                                                                                                    \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecKArg, cold)); \
    asm volatile("" : "+s"(C)); \
    unsigned hflags = H.flags; \
    int lane_t      = lane; \
    asm volatile("" : "+s"(hflags), "+v"(lane_t)); \
    spec_tile<SF, EMIS>(H, hflags, C, A.out, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_TILE
#undef SPEC_WG_KERNEL
}

} // namespace rt
