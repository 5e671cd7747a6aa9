#pragma once
// rt_step_scan.hip -- step mode with a length scan (rt_hip_plan_enable_length_scan): the step record at every plasma
// length n = 2 .. N from ONE forward march.
//
// With the forward method RayTrace_calc_ray walks the lengths ii = 1, 2, ... in order (Helper.h:430-441): its run with n
// lengths is the first n - 1 iterations of the outer loop of its run with N lengths, so the first 3 (n - 1) slots of the
// march record (gvl / evl / ivl) of the N-run are the whole record of the n-run.  What the n-run has and the N-run's record
// has not is the state with which the ray LEFT length j = n - 1: the scan instance of the march (rt_march.hip,
// MARCH_OPT_SCAN) stores it where the ray crosses the boundary, tile-wise (scan_bnd_off).  Which state serves length j
// (L = N - 1; e = the segment the ray escaped in, (n_done - 1) / 3 + 1 of its RecMeta):
//   not escaped, j < L      boundary j                          not escaped, j = L      the final RecMeta
//   escaped,     j < e      boundary j, the ray NOT escaped     escaped,     j >= e     the final RecMeta, escaped
// (a ray found outside by the first test of segment j + 1 has e = j + 1: for length j it has not escaped).
// Error -1 of length j is s.z^2 < 0.01 of that state (Helper.h:515); the seed factor is taken at the launch ray
// (Helper.h:530-533) and is 0 where the ray has escaped by j.
//
// rt_step_scan_kernel stands where rt_step_kernel stands and has its shape: one 16-wave work-group per CU, tiles from the
// eight sharded counters, lanes = rays; rt_tile_ray.inc and rt_tile_rec.inc are the text rt_step.hip includes, with
// SF = 0: the sub-segments are read slot by slot (rec_slot_lazy), which is what a long N needs.  The arithmetic of a slot
// is that of rt_tile_batch.inc for SF = 0 -- ase_step where the sub-segment is regular, ase_update otherwise and in the
// exact mode, the f64 product sum of the gain-only mode -- so every Iv_j[k] is the double rt_step_kernel<0, EMIS> computes
// on the prefix problem.  (The tile-wide choice between ase_step_f32 / ase_step / ase_update exists in the SF = 6
// instances only: with a run-time number of slots the choice is per slot, and a prefix of the slots takes the choices of
// the whole.)
//
// Per tile the lengths are taken in chunks of SCAN_LCH, unrolled under the wave-uniform test j <= L as the seed loops of
// rt_step_seeds.hip are: what is live per lane and length -- pixel, angle cell, the sum over k, and one bit each for "live",
// "carries the seed factor" and "a negative Iv seen" -- stays in registers with compile-time indices.  Per chunk and
// frequency batch the walk over the slots starts at slot 0: the slots below the chunk are integrated again without
// depositing, 3 LCH (c - 1) of them for chunk c.  Whenever the walk
// reaches a length (slot 3 j - 1) the kernel finishes Iv_j (gain-only: one exp_tab_vec), updates the length's sum over k
// and its sign / NaN test, and adds the E_v wave sum (rt_step_evsum.inc) to the length's accumulator in LDS; at the end of
// the chunk, per length, the I_ang add and the segmented nf scan (rt_wave_runs.inc, rt_wave_runscan.inc).  The kernel's
// shell -- LDS, prologue, epilogue, tile hand-out -- is the text rt_step_kernel includes (rt_step_wg.inc,
// rt_step_handout.inc), the grid-point seed factor the macro of place_ray (RT_SEED_GRID_FACTOR, rt_freq.hip).
//
// Failures follow the reference run once per length: error -1 at length j sets bit 1 of that length's code and keeps the
// ray out of record j; error -2 / -3 at length j removes the ray from record j only.  A ray that fails at any length is
// reported once, with the OR of its codes; DevCtl::len_code[j - 1] holds the code of length j.  The checking repeat keeps
// its two passes; the mark of a ray is one bit per length in a 32-bit word (FreqHot::bad is an array of words here),
// written by the one lane that holds the ray.
#include "rt_step_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int SCAN_LCH = 4; // lengths per pass over a tile

// what rt_step_scan_kernel reads beside the frequency kernel's block (through the constant address space, as the cold half)
struct ScanArg {
    const unsigned char *bnd; // boundary states of the march (scan_bnd_off)
    double *out;              // L blocks of `stride` doubles: E_v | nf at nf_off | I_ang at ang_off
    unsigned long long stride, nf_off, ang_off;
};
struct ScanKArg {
    FreqHot hot;
    FreqCold cold;
    ScanArg scan;
};
typedef const RT_CONST_AS ScanArg *ScanPtr;

// seed_factor (rt_math.h), statement by statement, with pchip_eval held to a call as the other kernels have it: inlined
// four times into this kernel it left the gain-only instance a 48-byte stack frame (that nothing read)
__device__ __forceinline__ double scan_seed_factor(const DevSeed &sd, double x, double y, double a, double b)
{
    double f = 0.0;
    if (x >= sd.x[0][0] && x <= sd.x[0][sd.dim[0] - 1] && y >= sd.x[1][0] && y <= sd.x[1][sd.dim[1] - 1] &&
        a >= sd.x[2][0] && a <= sd.x[2][sd.dim[2] - 1] && b >= sd.x[3][0] && b <= sd.x[3][sd.dim[3] - 1]) {
        double fx, fy, fa, fb;
        [[clang::noinline]] fx = pchip_eval(sd.dim[0], sd.x[0], sd.f[0], x);
        [[clang::noinline]] fy = pchip_eval(sd.dim[1], sd.x[1], sd.f[1], y);
        [[clang::noinline]] fa = pchip_eval(sd.dim[2], sd.x[2], sd.f[2], a);
        [[clang::noinline]] fb = pchip_eval(sd.dim[3], sd.x[3], sd.f[3], b);
        f = sd.f0 * fx * fy * fa * fb;
        f = f < 0.0 ? 0.0 : f;
    }
    return f;
}

template <bool EMIS>
__device__ __forceinline__ void step_scan_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, double *lds_iang, double *lds_ev,
                                               const double *tab, double *xpose, const unsigned tile, const int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH     = SCAN_LCH;
    const int L           = H.L;
    const int S           = L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned ridx   = tile * WAVE + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = false; // the forward method: rt_hip_plan_enable_length_scan takes no other
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool safe_check = (hflags & FQ_SAFE_CHECK) != 0, safe_skip = (hflags & FQ_SAFE_SKIP) != 0;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;
    unsigned *bad32       = reinterpret_cast<unsigned *>(H.bad);

    // ---- per-ray preamble, once: the final state of the ray, its launch ray (rt_tile_ray.inc) ----
    // (the launch ray is not kept across the tile: the seed factor below loads it, a failing ray loads its own when it is reported)
#define TILE_NEED_RAY false
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    if (__ballot(have) == 0ull)
        return;
    if (have && probe_on) {
        C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
        C->probe.steps[ridx] = steps;
    }
    // the segment the ray escaped in (never: L + 1)
    const int n_done = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
    const int e_seg  = (fl & F_ESCAPED) ? (n_done > 0 ? (n_done - 1) / RT_N_SUB + 1 : 1) : L + 1;
    // the seed factor at the launch ray, in place_ray's own arithmetic (it does not depend on the exit state with the
    // forward method); 0 without a seed
    double f0_launch = 0.0;
    if (have && (hflags & FQ_HAS_SEED)) { // place_ray's seed half for the forward method (Helper.h:523-533), its arithmetic and order
        if (!R.sf) {
            rt_ray launch = ray;
            float ta, tb;
            load_ray(R, ridx, launch, ta, tb, false);
            const DevSeed SD = load_cold(&C->seed);
            f0_launch        = scan_seed_factor(SD, (double) launch.x, (double) launch.y, (double) launch.a, (double) launch.b);
        } else {
            // the launch ray is a grid point: product of the tabulated factors (RT_SEED_GRID_FACTOR)
            RT_SEED_GRID_POINT(R, ridx)
            RT_SEED_GRID_FACTOR(f0_launch, C->seed.f0, R.sf, R.sin)
        }
    }

    // ---- the march record of this lane's ray (rt_tile_rec.inc; SF = 0: nothing to decode up front) ----
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
    (void) gs;
    (void) rs;
    (void) off;
    (void) all_small;
    (void) all_regular;
    (void) load_rows;
    (void) gv_nan; // (SF = 0 tests every frequency's lineshape values as it reads them)
    const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;
    const ConstF64 sfk = (ConstF64) (unsigned long long) H.seed_fk;

    // the lengths under which the checking pass found this ray failing: it stays out of their records
    const unsigned marked = (safe_skip && have) ? bad32[ridx] : 0u;
    unsigned code = 0u, marks = 0u; // OR of this ray's codes over the lengths; lengths (bit j - 1) it fails at with -2 / -3

    for (int j0 = 0; j0 < L; j0 += LCH) {
        // (what is live across the frequency loop per length: two cells and one sum; the seed factor is f0_launch or 0, the
        // sign test and `live` are one bit each)
        int pix[LCH], ang[LCH];
        double angsum[LCH];
        unsigned live = 0u, seeded = 0u, neg = 0u; // bit li: the ray is live at / carries its seed factor at / has had a negative Iv at length j0 + li + 1
        bool any_live = false;
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            const int j = j0 + li + 1; // the length, 1-based
            pix[li]     = -1;
            ang[li]     = -1;
            angsum[li]  = 0.0;
            if (j <= L) {
                // the state that serves length j
                RecMeta mj   = m;
                unsigned flj = fl;
                if (have && j < L && j < e_seg) {
                    const float *q = reinterpret_cast<const float *>(Q->bnd + scan_bnd_off(ridx, j, L));
                    mj.px          = q[0];
                    mj.py          = q[1];
                    mj.sx          = q[2];
                    mj.sy          = q[3];
                    mj.sz          = q[4];
                    flj            = fl & ~(unsigned) F_ESCAPED;
                }
                const bool e1 = have && (double) (mj.sz * mj.sz) < 0.01; // Helper.h:515
                if (e1 && !safe_skip) { // error -1 at this length: the ray is reported (once, below) and stays out of record j
                    code |= 1u << 1;
                    atomicOr(&H.ctl->len_code[j - 1], 1u << 1);
                }
                if (have && !e1) {
                    // pixel and angle cell of the exit state (the probe's exit ray is that of the whole run: j == L)
                    const unsigned pf = (hflags & ~(unsigned) (FQ_HAS_SEED | FQ_PROBE)) | (j == L ? (hflags & (unsigned) FQ_PROBE) : 0u);
                    const Placed P    = place_ray(pf, C, R, H.nx, backward, ridx, mj, flj, ray);
                    if (!(fl & F_SKIP) && !((marked >> (j - 1)) & 1u)) {
                        live |= 1u << li;
                        pix[li] = P.pix;
                        ang[li] = P.ang;
                        if (!(flj & F_ESCAPED)) // (an escaped ray's seed factor is 0, Helper.h:523-533)
                            seeded |= 1u << li;
                    }
                }
                any_live = any_live || ((live >> li) & 1u);
            }
            // (one placement after the other: interleaved, the four chains of loads of place_ray cost more registers than the
            // frequency loop has to spare)
            asm volatile("" ::: "memory");
        }
        if (__ballot(any_live) == 0ull)
            continue;

        const int s_lo = j0 * RT_N_SUB; // the slots below the chunk: integrated again, nothing deposited
        for (int kb = 0; kb < K; kb += VEC) {
            double acc[VEC]; // emission: the running Iv; gain-only: the running gl
            bool wnan[VEC];  // emission: a NaN or infinity among this frequency's lineshape values so far (0 * NaN on the CPU)
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                acc[v]  = 0.0;
                wnan[v] = false;
            }
            // one sub-segment: the SF = 0 text of rt_tile_batch.inc
            auto slot_step = [&](int s) {
                // (opaque: the slot addresses of a whole chunk, hoisted out of the frequency loop as invariants, cost eight
                // registers the loop does not have)
                asm volatile("" : "+s"(s));
                const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
                const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                const FVec w     = *reinterpret_cast<const FVec *>(row);
                if (EMIS) {
                    const float g1 = sl.g, e1 = sl.e;
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        wnan[v] = wnan[v] || !(fabsf(w.v[v]) <= FLT_MAX);
                    if (fabsf(g1) >= RT_RS_MIN && fabsf(g1) <= H.gs_cap && !exact_emis) {
                        const double r1 = div_fast((double) e1, (double) g1);
                        ase_step(acc, g1, r1, w.v, tab);
                    } else if (g1 != 0.0f || e1 != 0.0f) {
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            acc[v] = ase_update(acc[v], g1, e1, w.v[v], tab);
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        acc[v] += (double) sl.g * (double) w.v[v];
                }
            };
#pragma unroll 1
            for (int s = 0; s < s_lo; s++)
                slot_step(s);
#pragma unroll
            for (int li = 0; li < LCH; li++) {
                if (j0 + li < L) {
#pragma unroll 1
                    for (int t = 0; t < RT_N_SUB; t++)
                        slot_step(s_lo + li * RT_N_SUB + t);
                    // ---- the walk has reached length j0 + li + 1: its Iv ----
                    double Iv[VEC];
                    if (EMIS) {
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] = wnan[v] ? __builtin_nan("") : acc[v];
                    } else {
                        // Iv = f0 f[4][k] exp(gl); a wave none of whose lanes needs the exponential skips it (rt_tile_batch.inc)
                        const double f0 = ((seeded >> li) & 1u) ? f0_launch : 0.0;
                        bool need       = f0 != 0.0;
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            need = need || acc[v] > 700.0 || acc[v] != acc[v];
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] = f0 * sfk[kb + v];
                        if (__ballot(need) != 0ull) {
                            double eg[VEC];
                            exp_tab_vec(acc, tab, eg);
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                Iv[v] *= eg[v];
                        }
                    }
#pragma unroll
                    for (int v = 0; v < VEC; v++) {
                        neg |= Iv[v] < 0.0 ? 1u << li : 0u; // (min over k of Iv negative, NaNs ignored: error -2, Helper.h:582-594)
                        angsum[li] += dv2[kb + v] * Iv[v]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                    }
                    if (!safe_check) { // the checking pass of a failing run integrates without depositing
                        // E_v of this length: the wave sum over the lanes that deposit at this length, into the length's accumulator
                        const bool dep = pix[li] >= 0;
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX (j0 + li) * Kp + kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
                    }
                }
            }
        }
        // ---- per length of the chunk: the failure test (Helper.h:582-594), the I_ang add, the segmented nf scan ----
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            if (j0 + li < L) {
                const int jb       = j0 + li; // block and bit of this length
                const bool bad_neg = ((neg >> li) & 1u) != 0u, bad_nan = angsum[li] != angsum[li];
                const bool failing = bad_neg || bad_nan;
                if (((live >> li) & 1u) && failing && !safe_skip) {
                    const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                    code |= c;
                    marks |= 1u << jb;
                    atomicOr(&H.ctl->len_code[jb], c);
                }
                if (!safe_check) {
                    double *blk = Q->out + (size_t) jb * (size_t) Q->stride;
                    // a failing ray adds nothing to the record of this length (RayTraceImageCPU.cpp:29-36)
                    if (ang[li] >= 0 && !failing) {
                        if (lds_iang)
                            unsafeAtomicAdd(&lds_iang[jb * seeds_ang_stride(H.n_ang) + ang[li]], angsum[li]);
                        else
                            unsafeAtomicAdd(&blk[Q->ang_off + (unsigned) ang[li]], angsum[li]);
                    }
                    // nf: the segmented scan over the runs of equal pixel AT THIS LENGTH (rt_wave_runs.inc, rt_wave_runscan.inc)
                    const int px   = pix[li];
                    const bool dep = px >= 0;
#define RUNS_PIX px
#define RUNS_DEPOSITS dep
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
                    double a = (dep && !failing) ? angsum[li] * H.scale : 0.0;
#include "rt_wave_runscan.inc"
                    if (tail && a != 0.0)
                        unsafeAtomicAdd(&blk[Q->nf_off + (unsigned) px], a);
                }
            }
        }
    }
    if (code) { // one report per ray, whatever the number of lengths it fails at
        report_failure(code);
        if (safe_check && marks)
            bad32[ridx] = marks; // the lane that holds the ray writes all its bits
    }
}

// The shell of rt_step_kernel (rt_step_wg.inc, rt_step_handout.inc) with one record per length: per length an I_ang
// histogram, seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.
template <bool EMIS>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_step_scan_kernel(const ScanKArg A)
{
    const FreqHot &H = A.hot;
#define STEP_WG_NREC H.L
#define STEP_WG_ANG_STRIDE seeds_ang_stride(n_ang)
#define STEP_WG_ANG_ZERO n_rec * ang_stride
#define STEP_WG_RECORD(r) double *blk = A.scan.out + (size_t) r * (size_t) A.scan.stride;
#define STEP_WG_EV(r, c) blk[c]
#define STEP_WG_IANG(r, c) blk[A.scan.ang_off + c]
#define STEP_WG_PROLOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_PROLOGUE
    const int lane = lane_id();
    // the cold half and the scan block of the argument block, the flag word and the lane number opaque per tile
#define HANDOUT_TILES_PER_FETCH (EMIS ? FREQ_TILES_PER_FETCH_EMIS : FREQ_TILES_PER_FETCH_GAIN)
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanKArg, cold));            \
    ScanPtr Q = (ScanPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanKArg, scan));             \
    asm volatile("" : "+s"(C), "+s"(Q));                                                                                               \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    asm volatile("" : "+s"(hflags), "+v"(lane_t));                                                                                     \
    step_scan_tile<EMIS>(H, hflags, C, Q, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
#include "rt_step_handout.inc"
#undef HANDOUT_TILES_PER_FETCH
#undef HANDOUT_TILE
#define STEP_WG_EPILOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_EPILOGUE
#undef STEP_WG_NREC
#undef STEP_WG_ANG_STRIDE
#undef STEP_WG_ANG_ZERO
#undef STEP_WG_RECORD
#undef STEP_WG_EV
#undef STEP_WG_IANG
}

} // namespace rt
