#pragma once
// rt_step_rscan.hip -- step mode with a suffix scan (rt_hip_plan_enable_suffix_scan): the step record of the run of the LAST
// n lengths, n = 2 .. N, from ONE backward march.
//
// With the backward method RayTrace_calc_ray starts at the launch ray and walks the lengths ii = N - 1, N - 2, ..., 1
// (Helper.h:430-441): its first n - 1 outer iterations are the whole run of the problem that holds gain[0] and the last
// n - 1 lengths (problem.suffix_lengths), so slots 3 (N - n) .. 3 (N - 1) - 1 of the march record of the N-run are the
// whole record of that run, and the state it ends with is the state with which the ray left its m = n - 1 first marched
// segments: boundary m of the scan instance of the march (rt_march.hip, MARCH_OPT_SCAN: the store is indexed by the number
// of segments marched, whatever the method).  Which state serves record n (L = N - 1; e = the marched segment the ray
// escaped in, (n_done - 1) / 3 + 1 of its RecMeta, L + 1 if never):
//   not escaped, m < L      boundary m                          not escaped, m = L      the final RecMeta
//   escaped,     m < e      boundary m, the ray NOT escaped     escaped,     m >= e     the final RecMeta, escaped
// Error -1 of record n is s.z^2 < 0.01 of that state (Helper.h:515); the seed factor (gain-only mode) is taken at that
// state's position and exit angles (Helper.h:525-529) and is 0 where the ray has escaped by m.  The backward method
// deposits at the LAUNCH ray (RayTraceImageCPU.cpp:37-39): pixel, angle cell and the runs of equal pixel of a tile are the
// same for every record and are taken once.
//
// rt_step_rscan_kernel stands where rt_step_scan_kernel stands and has its shell (rt_step_wg.inc, rt_step_handout.inc, one
// 16-wave work-group per CU, the eight sharded counters, the same launch bounds) and its tile text (rt_tile_ray.inc,
// rt_tile_rec.inc with SF = 0, rec_slot_lazy).  What differs is the walk.  The recurrence of a suffix starts with Iv = 0 at
// its own first slot, so the suffixes do not share a running value as the prefixes do -- but in emission mode they share
// everything of a slot that is expensive: e^gl - 1 and rs depend on the slot alone (ase_step, rt_freq.hip), the update
// is Iv = fma(em1, Iv + rs, Iv), one add and one fma per accumulator.  The suffixes are taken in chunks of LCH start
// segments a0 .. a0 + LCH - 1 (start segment a is record n = N - a): per frequency batch ONE walk over slots 3 a0 .. S - 1 with LCH
// accumulators of VEC doubles in registers, accumulator i joining at slot 3 (a0 + i).  The joining part is unrolled so that
// the number of live accumulators is a compile-time count; no slot is integrated twice inside a chunk, chunk c = 0, 1, ...
// walks 3 LCH c slots fewer than the first.  Every Iv_n[k] is the double rt_step_kernel<0, EMIS> computes on the suffix problem:
// ase_factor below is ase_step up to its last line, irregular sub-segments and the exact mode take ase_update per
// accumulator, the gain-only mode the same f64 product sum and one ballot-skipped exp_tab_vec per record.
//
// The chunk: the launch bounds allow 128 VGPRs (four waves per SIMD).  An accumulator is 8 of them, the sum over k of a
// record 2, its seed factor (gain-only) 2; pixel, angle cell and run structure are held once.  Emission takes
// RSCAN_LCH_EMIS = 4 (118 VGPRs, no scratch), gain-only RSCAN_LCH_GAIN = 3 (117 VGPRs, no scratch; with four the instance
// is at 126 and keeps a 48-byte frame, as rt_step_scan_kernel once did with a fourth inlined seed factor).
// profiles/suffix_scan_kernel_resources.txt has what the compiler made of both.
//
// Failures follow the reference run once per record, as in rt_step_scan.hip: error -1 under record n sets bit 1 of that
// record's code and keeps the ray out of record n; error -2 / -3 under record n removes the ray from record n only.  A ray
// that fails anywhere is reported once, with the OR of its codes; DevCtl::len_code[n - 2] holds the code of record n.  The
// mark of the checking repeat is one bit per record in a 32-bit word.  The probe's exit ray, flags and steps are those of
// the whole run.
#include "rt_step_scan.hip"

#include <type_traits>

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int RSCAN_LCH_EMIS = 4, RSCAN_LCH_GAIN = 3; // suffixes (start segments) per walk over a tile

// e^gl - 1 of a regular sub-segment for VEC frequencies: ase_step (rt_freq.hip) up to its last line, statement by
// statement; apply(j, em1) stands where ase_step has Iv[j] = fma(em1, Iv[j] + rs, Iv[j]) and does that for every accumulator
// that takes the factor, so each of them is ase_step's Iv.  (The factor is handed over frequency by frequency, as ase_step
// consumes it: four of them held beside the accumulators are six more registers alive across the updates.)
template <typename Apply> __device__ __forceinline__ void ase_factor(const float gs, const float (&w)[VEC], const double *tab, Apply apply)
{
    const double L2E   = 369.3299304675746;     // 256 / ln 2
    const double LN2_N = 0.0027076061740622863; // ln 2 / 256
    const double MAGIC = 0x1.8p52;              // adding it leaves rint(.) in the low mantissa bits
    double rq[VEC], T[VEC];
    int m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        const double x = (double) (gs * w[j]);
        double t       = fma(x, L2E, MAGIC);
        const int n    = __double2loint(t);
        t -= MAGIC;
        rq[j] = fma(-t, LN2_N, x);
        T[j]  = tab[n & (EXP_TAB - 1)];
        m[j]  = n >> 8;
    }
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        double q = fma(rq[j], 1.0 / 6.0, 0.5);
        q        = fma(rq[j], q, 1.0);
        rq[j] *= q;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        int hi; // exponent field += m (ase_step's instruction)
        asm("v_lshl_add_u32 %0, %1, 20, %2" : "=v"(hi) : "v"(m[j]), "v"(__double2hiint(T[j])));
        const double S = __hiloint2double(hi, __double2loint(T[j]));
        apply(j, fma(S, rq[j], S - 1.0));
    }
}

// ase_update (rt_freq.hip) held to a call, as scan_seed_factor holds pchip_eval: the update of the irregular sub-segments
// and of the exact mode, the same statements and hence the same double
static __device__ __attribute__((noinline)) double ase_update_call(double Iv, float gs, float es, float w, const double *tab)
{
    return ase_update(Iv, gs, es, w, tab);
}

// scan_seed_factor (rt_step_scan.hip), statement by statement, on a seed that stays in the argument block: every table
// pointer and dimension is read through the constant address space where it is used, not as a copy of the whole DevSeed
// held in scalar registers across the four calls (with the copy the kernel kept a stack frame that nothing read).  The
// kernels that carry the seeds of a suffix scan take it (rt_step_rscan_ase_seeds.hip, rt_step_rscan_seeds.hip).
__device__ __forceinline__ double rscan_seed_factor(const RT_CONST_AS DevSeed *sd, double x, double y, double a, double b)
{
    auto xs  = [&](int d) { return (ConstF64) (unsigned long long) sd->x[d]; };
    auto fs  = [&](int d) { return reinterpret_cast<const double *>((unsigned long long) sd->f[d]); };
    double f = 0.0;
    if (x >= xs(0)[0] && x <= xs(0)[sd->dim[0] - 1] && y >= xs(1)[0] && y <= xs(1)[sd->dim[1] - 1] && a >= xs(2)[0] &&
        a <= xs(2)[sd->dim[2] - 1] && b >= xs(3)[0] && b <= xs(3)[sd->dim[3] - 1]) {
        double fx, fy, fa, fb;
        [[clang::noinline]] fx = pchip_eval(sd->dim[0], reinterpret_cast<const double *>((unsigned long long) sd->x[0]), fs(0), x);
        [[clang::noinline]] fy = pchip_eval(sd->dim[1], reinterpret_cast<const double *>((unsigned long long) sd->x[1]), fs(1), y);
        [[clang::noinline]] fa = pchip_eval(sd->dim[2], reinterpret_cast<const double *>((unsigned long long) sd->x[2]), fs(2), a);
        [[clang::noinline]] fb = pchip_eval(sd->dim[3], reinterpret_cast<const double *>((unsigned long long) sd->x[3]), fs(3), b);
        f = sd->f0 * fx * fy * fa * fb;
        f = f < 0.0 ? 0.0 : f;
    }
    return f;
}

template <bool EMIS>
__device__ __forceinline__ void step_rscan_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, double *lds_iang, double *lds_ev,
                                                const double *tab, double *xpose, const unsigned tile, const int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH     = EMIS ? RSCAN_LCH_EMIS : RSCAN_LCH_GAIN;
    const int L           = H.L;
    const int S           = L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned ridx   = tile * WAVE + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = true; // the backward method: rt_hip_plan_enable_suffix_scan takes no other
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool safe_check = (hflags & FQ_SAFE_CHECK) != 0, safe_skip = (hflags & FQ_SAFE_SKIP) != 0;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;
    unsigned *bad32       = reinterpret_cast<unsigned *>(H.bad);

    // ---- per-ray preamble, once: the final state of the ray, its launch ray (rt_tile_ray.inc) ----
    // (the launch ray is not kept across the tile: the placement below loads it, a failing ray loads its own when it is reported)
#define TILE_NEED_RAY false
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    if (__ballot(have) == 0ull)
        return;
    if (have && probe_on) {
        C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
        C->probe.steps[ridx] = steps;
    }
    // the marched segment the ray escaped in (never: L + 1)
    const int n_done = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
    const unsigned flags_steps = m.flags_steps; // (what the walk needs of the final state; the rest is read again per chunk)
    const int e_seg  = (fl & F_ESCAPED) ? (n_done > 0 ? (n_done - 1) / RT_N_SUB + 1 : 1) : L + 1;
    // pixel and angle cell of the LAUNCH ray, one placement for all records (the seed factor is per record, below; the
    // probe's exit ray is that of the whole run, written as rt_step_kernel writes it: not under error -1)
    int pix = -1, ang = -1;
    if (have) {
        const unsigned pf = (hflags & ~(unsigned) (FQ_HAS_SEED | FQ_PROBE)) | (err1 ? 0u : (hflags & (unsigned) FQ_PROBE));
        rt_ray launch     = ray;
        if (!(hflags & FQ_OWN_CELLS)) { // (own cells: the grid point is the placement, no coordinate is read)
            float ta, tb;
            load_ray(R, ridx, launch, ta, tb, false);
        }
        const Placed P    = place_ray(pf, C, R, H.nx, backward, ridx, m, fl, launch);
        if (!(fl & F_SKIP)) {
            pix = P.pix;
            ang = P.ang;
        }
    }
    // the runs of equal pixel, one structure for all records: the last lane of a run owns the run's total of every record
    // (a record's own depositing lanes are a subset of the run: the others add 0.0)
    const bool has_pix = pix >= 0;
#define RUNS_PIX pix
#define RUNS_DEPOSITS has_pix
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
    (void) pix_prev;

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

    // the records under which the checking pass found this ray failing: it stays out of them
    const unsigned marked = (safe_skip && have) ? bad32[ridx] : 0u;
    unsigned code = 0u, marks = 0u; // OR of this ray's codes over the records; records (bit n - 2) it fails under with -2 / -3

    for (int a0 = 0; a0 < L; a0 += LCH) {
        // accumulator i of the chunk: the suffix whose first slot is 3 (a0 + i) -- the run of m = L - (a0 + i) marched
        // segments, record n = m + 1, block and bit m - 1
        double angsum[LCH], f0[LCH];
        unsigned live = 0u, neg = 0u; // bit i: the ray is live under / has had a negative Iv under the record of accumulator i
        // (the final state again, from memory: five registers that need not live across the frequency loops)
        RecMeta mc = { 0, 0, 0, 0, 1, 0 };
        if (have)
            mc = *reinterpret_cast<const RecMeta *>(rec + rec_meta_off(rrec, S, H.rec_stride));
#pragma unroll
        for (int i = 0; i < LCH; i++) {
            angsum[i] = 0.0;
            f0[i]     = 0.0;
            if (a0 + i < L) {
                const int mseg = L - (a0 + i);
                // the state that serves this record
                float spx = mc.px, spy = mc.py, ssx = mc.sx, ssy = mc.sy, ssz = mc.sz;
                bool esc  = (fl & F_ESCAPED) != 0u;
                if (have && mseg < L && mseg < e_seg) {
                    const float *q = reinterpret_cast<const float *>(Q->bnd + scan_bnd_off(ridx, mseg, L));
                    spx            = q[0];
                    spy            = q[1];
                    ssx            = q[2];
                    ssy            = q[3];
                    ssz            = q[4];
                    esc            = false;
                }
                const bool e1 = have && (double) (ssz * ssz) < 0.01; // Helper.h:515
                if (e1 && !safe_skip) { // error -1 under this record: the ray is reported (once, below) and stays out of it
                    code |= 1u << 1;
                    atomicOr(&H.ctl->len_code[mseg - 1], 1u << 1);
                }
                if (have && !e1 && !(fl & F_SKIP) && !((marked >> (mseg - 1)) & 1u)) {
                    live |= 1u << i;
                    // the seed factor at this state's position and exit angles (place_ray's backward half, Helper.h:518-529);
                    // 0 where the ray has escaped by m
                    if (!EMIS && (hflags & FQ_HAS_SEED) && !esc) {
                        const float ea   = atanf_flt32_kernel(ssx / ssz) * 1e3f;
                        const float eb   = atanf_flt32_kernel(ssy / ssz) * 1e3f;
                        const DevSeed SD = load_cold(&C->seed);
                        f0[i]            = scan_seed_factor(SD, (double) spx, (double) spy, (double) ea, (double) eb);
                    }
                }
            }
            // (one state after the other, as rt_step_scan.hip places one length after the other)
            asm volatile("" ::: "memory");
        }
        if (__ballot(live != 0u) == 0ull)
            continue;

        for (int kb = 0; kb < K; kb += VEC) {
            double acc[LCH][VEC]; // emission: the running Iv of every suffix; gain-only: its running gl
            unsigned wnan = 0u;   // emission, bit i * VEC + v: a NaN or infinity among frequency v's lineshape values since suffix i began
#pragma unroll
            for (int i = 0; i < LCH; i++) {
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[i][v] = 0.0;
            }
            // one sub-segment for the first NL accumulators: the SF = 0 text of rt_tile_batch.inc, its factor taken once
            auto slot_step = [&](auto nl_tag, int s) {
                constexpr int NL = decltype(nl_tag)::value;
                // (opaque, as in rt_step_scan.hip: no slot addresses hoisted out of the frequency loop)
                asm volatile("" : "+s"(s));
                const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, flags_steps, backward);
                const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                const FVec w     = *reinterpret_cast<const FVec *>(row);
                if (EMIS) {
                    const float g1 = sl.g, e1 = sl.e;
                    unsigned wn = 0u;
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        wn |= !(fabsf(w.v[v]) <= FLT_MAX) ? 1u << v : 0u;
                    constexpr unsigned spread = NL >= 4 ? 0x1111u : NL == 3 ? 0x111u : NL == 2 ? 0x11u : 0x1u;
                    static_assert(VEC == 4 && LCH <= 4, "wnan keeps VEC bits per accumulator, four accumulators at most");
                    wnan |= wn * spread;
                    if (fabsf(g1) >= RT_RS_MIN && fabsf(g1) <= H.gs_cap && !exact_emis) {
                        const double r1 = div_fast((double) e1, (double) g1);
                        ase_factor(g1, w.v, tab, [&](const int v, const double em1) {
#pragma unroll
                            for (int i = 0; i < NL; i++)
                                acc[i][v] = fma(em1, acc[i][v] + r1, acc[i][v]);
                        });
                    } else if (g1 != 0.0f || e1 != 0.0f) {
                        // (ase_update_call: inlined NL * VEC times into each of the
                        // five copies of this text the rare path set the register count -- 128 VGPRs and 68 spilled at
                        // four accumulators, 118 and none with the call)
#pragma unroll
                        for (int i = 0; i < NL; i++) {
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                acc[i][v] = ase_update_call(acc[i][v], g1, e1, w.v[v], tab);
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < NL; i++) {
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            acc[i][v] += (double) sl.g * (double) w.v[v];
                    }
                }
            };
            // the joining part: segment a0 + I is walked with accumulators 0 .. I (a count the compiler knows: a loop variable
            // is no template argument, hence the four statements)
#define RSCAN_JOIN(I)                                                                                            \
    if (I < LCH && a0 + I < L) {                                                                                 \
        _Pragma("unroll 1") for (int t = 0; t < RT_N_SUB; t++)                                                   \
            slot_step(std::integral_constant<int, (I < LCH ? I + 1 : LCH)>{}, (a0 + I) * RT_N_SUB + t);          \
    }
            RSCAN_JOIN(0)
            RSCAN_JOIN(1)
            RSCAN_JOIN(2)
            RSCAN_JOIN(3)
#undef RSCAN_JOIN
            // ... and the segments behind the chunk's last start with all of them
#pragma unroll 1
            for (int s = (a0 + LCH) * RT_N_SUB; s < S; s++)
                slot_step(std::integral_constant<int, LCH>{}, s);

            // ---- the walk has reached the end of the record: Iv of every suffix of the chunk ----
#pragma unroll
            for (int i = 0; i < LCH; i++) {
                if (a0 + i < L) {
                    double Iv[VEC];
                    if (EMIS) {
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] = ((wnan >> (i * VEC + v)) & 1u) ? __builtin_nan("") : acc[i][v];
                    } else {
                        // Iv = f0 f[4][k] exp(gl); a wave none of whose lanes needs the exponential skips it (rt_tile_batch.inc)
                        bool need = f0[i] != 0.0;
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            need = need || acc[i][v] > 700.0 || acc[i][v] != acc[i][v];
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] = f0[i] * sfk[kb + v];
                        if (__ballot(need) != 0ull) {
                            double eg[VEC];
                            exp_tab_vec(acc[i], tab, eg);
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                Iv[v] *= eg[v];
                        }
                    }
#pragma unroll
                    for (int v = 0; v < VEC; v++) {
                        neg |= Iv[v] < 0.0 ? 1u << i : 0u; // (min over k of Iv negative, NaNs ignored: error -2, Helper.h:582-594)
                        angsum[i] += dv2[kb + v] * Iv[v]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                    }
                    if (!safe_check) { // the checking pass of a failing run integrates without depositing
                        // E_v of this record: the wave sum over the lanes that deposit into it, into the record's accumulator
                        const bool dep = has_pix && ((live >> i) & 1u);
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX (L - 1 - (a0 + i)) * Kp + kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
                    }
                }
            }
        }
        // ---- per record of the chunk: the failure test (Helper.h:582-594), the I_ang add, the segmented nf scan ----
#pragma unroll
        for (int i = 0; i < LCH; i++) {
            if (a0 + i < L) {
                const int jb       = L - 1 - (a0 + i); // block and bit of this record
                const bool lv      = ((live >> i) & 1u) != 0u;
                const bool bad_neg = ((neg >> i) & 1u) != 0u, bad_nan = angsum[i] != angsum[i];
                const bool failing = bad_neg || bad_nan;
                if (lv && failing && !safe_skip) {
                    const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                    code |= c;
                    marks |= 1u << jb;
                    atomicOr(&H.ctl->len_code[jb], c);
                }
                if (!safe_check) {
                    double *blk = Q->out + (size_t) jb * (size_t) Q->stride;
                    // a failing ray adds nothing to this record (RayTraceImageCPU.cpp:29-36)
                    if (ang >= 0 && lv && !failing) {
                        if (lds_iang)
                            unsafeAtomicAdd(&lds_iang[jb * seeds_ang_stride(H.n_ang) + ang], angsum[i]);
                        else
                            unsafeAtomicAdd(&blk[Q->ang_off + (unsigned) ang], angsum[i]);
                    }
                    // nf: the segmented scan over the runs of equal pixel of the tile (rt_wave_runscan.inc), one atomic per run tail
                    double a = (has_pix && lv && !failing) ? angsum[i] * H.scale : 0.0;
#include "rt_wave_runscan.inc"
                    if (tail && a != 0.0)
                        unsafeAtomicAdd(&blk[Q->nf_off + (unsigned) pix], a);
                }
            }
        }
    }
    if (code) { // one report per ray, whatever the number of records it fails under
        report_failure(code);
        if (safe_check && marks)
            bad32[ridx] = marks; // the lane that holds the ray writes all its bits
    }
}

// The shell of rt_step_scan_kernel, word for word: one record per length, per record an I_ang histogram,
// seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.
template <bool EMIS>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, EMIS ? FREQ_WAVES : FREQ_WAVES_SEED) rt_step_rscan_kernel(const ScanKArg A)
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
    step_rscan_tile<EMIS>(H, hflags, C, Q, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
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
