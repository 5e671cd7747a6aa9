#pragma once
// rt_step_rscan_seeds.hip -- step mode of a SEEDED backward plan with a suffix scan AND the seeds of that scan
// (rt_hip_plan_set_suffix_seeds): the step record of every seed beam s < n_seed <= RT_N_SEED_MAX of the run of the LAST n
// lengths, n = 2 .. N, from ONE backward march.
//
// The premises are those of rt_step_scan_seeds.hip and rt_step_rscan.hip: neither the march nor the boundary states depend on
// the seed, which enters as Iv[k] = f0_s f_s[4][k] exp(gl[k]) only, and the backward run of N lengths begins with the run of
// the last n.  The march is the suffix-scan march of the seeded plan unchanged (MODE 0, MARCH_OPT_SCAN);
// rt_step_rscan_seeds_kernel stands where rt_step_rscan_kernel<false> stands and leaves n_seed L records, record
// (s, n) = block s L + (n - 2) -- a seed's curve is contiguous, the layout of rt_step_scan_seeds.hip, whose argument block
// this kernel takes:
//   (s, n)   what rt_step_rscan_kernel<false> leaves for n on a plan of the same problem created with seed s:
//            Iv[k] = f0_{s,n} f_s[4][k] exp(gl_n[k]), multiplied in that kernel's order, gl_n the f64 product sum over the
//            suffix's slots in slot order, the seed factor at the position and exit angles of the state that serves record n
//            (the table of rt_step_rscan.hip; rscan_seed_factor), 0 where the ray has escaped by m = n - 1; the plan's scale
// The creation seed is not among the seeds (rt_step_scan_seeds.hip).  The shell is that of every step pass (rt_step_wg.inc,
// rt_step_handout.inc), rt_tile_ray.inc / rt_tile_rec.inc with SF = 0; the backward method deposits at the LAUNCH ray, so
// pixel, angle cell and the runs of equal pixel are taken once per tile for all records.
//
// The walk is the seed half of rt_step_rscan_ase_seeds.hip: chunks of RSCAN_SEEDS_LCH start segments; per chunk and record
// the serving state (boundary m, or the final RecMeta read again from memory) and one seed factor per seed; per frequency
// batch ONE gl walk with the joining part of rt_step_rscan.hip and one ballot-skipped exp_tab_vec per record for all seeds;
// per (seed, record) the sum over k, the failure test, the I_ang add and the segmented nf scan.  What is held across the
// frequency loop per accumulator is the running gl (8 registers) and per seed a factor and a sum (4 each).  With three start
// segments per walk at two seeds the kernel takes 127 VGPRs, none spilled, no scratch and no stack frame -- four waves per
// SIMD; with two it takes 123, with four it spills five and keeps 32 bytes of scratch.  The marks of the checking repeat are
// read and written chunk by chunk: held across the walks as rt_step_scan_seeds.hip holds them (two 64-bit words) the kernel
// spilled four VGPRs at three segments (profiles/suffix_seeds_kernel_resources.txt has what the compiler made of each).
//
// A ray is live for (s, n) exactly when rt_step_rscan_kernel<false> holds it live for n: it has a record, the serving state
// is not under error -1, it is not marked F_SKIP and the checking repeat has not marked it under (s, n).
//
// Failures follow the reference run once per (seed, n): error -1 of the state that serves n keeps the ray out of every
// (s, n) and sets bit 1 in each of their codes; error -2 / -3 under (s, n) removes the ray from (s, n) only.  A failing ray
// is reported once, with the OR of its codes; DevCtl::seed_len_code[s][n - 2] holds the code of (s, n).  The mark of the
// checking repeat is that of rt_step_scan_seeds.hip: bit 32 s + (n - 2) of a 64-bit word per ray, written by the lane that
// holds the ray.
#include "rt_step_rscan.hip"
#include "rt_step_scan_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int RSCAN_SEEDS_LCH = 3; // suffixes (start segments) per walk over a tile

__device__ __forceinline__ void step_rscan_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, ScanSetPtr Z, const int n_seed,
                                                      double *lds_iang, double *lds_ev, const double *tab, double *xpose, const unsigned tile,
                                                      const int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH     = RSCAN_SEEDS_LCH;
    constexpr int NS      = RT_N_SEED_MAX;
    const int L           = H.L;
    const int S           = L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned ridx   = tile * WAVE + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = true; // the backward method: the suffix scan takes no other
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool safe_check = (hflags & FQ_SAFE_CHECK) != 0, safe_skip = (hflags & FQ_SAFE_SKIP) != 0;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;
    unsigned long long *bad64 = reinterpret_cast<unsigned long long *>(H.bad); // one word per ray: bit 32 s + (n - 2)

    // ---- per-ray preamble, once: the final state of the ray, its launch ray (rt_tile_ray.inc) ----
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
    // pixel and angle cell of the LAUNCH ray, one placement for all records, as step_rscan_tile takes it (the seed factors are
    // per record, below; the probe's exit ray is that of the whole run: not under error -1)
    int pix = -1, ang = -1;
    if (have) {
        const unsigned pf = (hflags & ~(unsigned) (FQ_HAS_SEED | FQ_PROBE)) | (err1 ? 0u : (hflags & (unsigned) FQ_PROBE));
        rt_ray launch     = ray;
        if (!(hflags & FQ_OWN_CELLS)) { // (own cells: the grid point is the placement, no coordinate is read)
            float ta, tb;
            load_ray(R, ridx, launch, ta, tb, false);
        }
        const Placed P = place_ray(pf, C, R, H.nx, backward, ridx, m, fl, launch);
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
    (void) gv_nan;
    (void) exact_emis;
    const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;

    unsigned code = 0u; // OR of this ray's codes over seeds and n
    // (the marks of the checking repeat are read and written chunk by chunk, a chunk's records are its own: two 64-bit words
    // that need not live across the frequency loops, as rt_step_rscan_ase_seeds.hip keeps its four)

    static_assert(NS * LCH <= 16, "live and neg keep one bit per (seed, accumulator)");
    for (int a0 = 0; a0 < L; a0 += LCH) {
        // accumulator i of the chunk: the suffix whose first slot is 3 (a0 + i) -- the run of m = L - (a0 + i) marched
        // segments, record n = m + 1, block (within a seed's curve) and bit m - 1
        double angsum[NS][LCH], f0[NS][LCH];
        unsigned live = 0u, neg = 0u; // bit s * LCH + i: the ray is live under / has had a negative Iv under record (s, .) of accumulator i
#pragma unroll
        for (int i = 0; i < LCH; i++) {
#pragma unroll
            for (int s = 0; s < NS; s++) {
                angsum[s][i] = 0.0;
                f0[s][i]     = 0.0;
            }
            if (a0 + i < L) {
                const int mseg = L - (a0 + i);
                // the state that serves this record: a boundary state or the final one, which begin with the same five floats
                // (position, direction) -- read where it is needed, so that no state is held across the seed factors
                static_assert(offsetof(RecMeta, px) == 0 && offsetof(RecMeta, sz) == 16, "a boundary state and a RecMeta begin alike");
                const bool at_bnd = mseg < L && mseg < e_seg;
                const bool esc    = !at_bnd && (fl & F_ESCAPED) != 0u;
                float spx = 0.0f, spy = 0.0f, ssx = 0.0f, ssy = 0.0f, ssz = 1.0f;
                if (have) {
                    const float *q = reinterpret_cast<const float *>(at_bnd ? Q->bnd + scan_bnd_off(ridx, mseg, L)
                                                                            : rec + rec_meta_off(rrec, S, H.rec_stride));
                    spx            = q[0];
                    spy            = q[1];
                    ssx            = q[2];
                    ssy            = q[3];
                    ssz            = q[4];
                }
                const bool e1 = have && (double) (ssz * ssz) < 0.01; // Helper.h:515
                if (e1 && !safe_skip) { // error -1 under n, whatever the seed: reported (once, below), out of every record (s, n)
                    code |= 1u << 1;
#pragma unroll
                    for (int s = 0; s < NS; s++)
                        if (s < n_seed)
                            atomicOr(&H.ctl->seed_len_code[s][mseg - 1], 1u << 1);
                }
                if (have && !e1 && !(fl & F_SKIP)) {
                    // the (seed, n) pairs under which the checking pass found this ray failing: it stays out of their records
                    const unsigned long long marked = safe_skip ? bad64[ridx] : 0ull;
                    unsigned lv = 0u;
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (s < n_seed && !((marked >> (32 * s + mseg - 1)) & 1ull))
                            lv |= 1u << (s * LCH + i);
                    }
                    live |= lv;
                    // the seed factors at this state's position and exit angles (place_ray's backward half, Helper.h:518-529);
                    // 0 where the ray has escaped by m
                    if (lv && !esc) {
                        const float ea = atanf_flt32_kernel(ssx / ssz) * 1e3f;
                        const float eb = atanf_flt32_kernel(ssy / ssz) * 1e3f;
                        // (one copy of the text per accumulator: the seeds in a loop the compiler does not unroll, the factor
                        // filed by selects -- rt_step_rscan_ase_seeds.hip)
#pragma unroll 1
                        for (int s = 0; s < n_seed; s++) {
                            const double f = rscan_seed_factor(&Z->tabs.seed[s], (double) spx, (double) spy, (double) ea, (double) eb);
#pragma unroll
                            for (int t = 0; t < NS; t++)
                                f0[t][i] = t == s ? f : f0[t][i];
                        }
                    }
                }
            }
            // (one state after the other, as rt_step_scan.hip places one length after the other)
            asm volatile("" ::: "memory");
        }
        if (__ballot(live != 0u) == 0ull)
            continue;

        for (int kb = 0; kb < K; kb += VEC) {
            double acc[LCH][VEC]; // the running gl of every suffix
#pragma unroll
            for (int i = 0; i < LCH; i++) {
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[i][v] = 0.0;
            }
            // one sub-segment for the first NL accumulators: the gain-only SF = 0 text of rt_tile_batch.inc
            auto slot_step = [&](auto nl_tag, int s) {
                constexpr int NL = decltype(nl_tag)::value;
                asm volatile("" : "+s"(s)); // (opaque, as in rt_step_scan.hip: no slot addresses hoisted out of the frequency loop)
                const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, flags_steps, backward);
                const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                const FVec w     = *reinterpret_cast<const FVec *>(row);
#pragma unroll
                for (int i = 0; i < NL; i++) {
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        acc[i][v] += (double) sl.g * (double) w.v[v];
                }
            };
            // the joining part: segment a0 + I is walked with accumulators 0 .. I (rt_step_rscan.hip)
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

            // ---- the walk has reached the end of the record: exp(gl) once per suffix, then Iv per seed ----
#pragma unroll
            for (int i = 0; i < LCH; i++) {
                if (a0 + i < L) {
                    // a wave none of whose lanes needs the exponential skips it (rt_tile_batch.inc)
                    bool need = false;
#pragma unroll
                    for (int s = 0; s < NS; s++)
                        need = need || f0[s][i] != 0.0;
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        need = need || acc[i][v] > 700.0 || acc[i][v] != acc[i][v];
                    const bool with_exp = __ballot(need) != 0ull;
                    double eg[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        eg[v] = 1.0;
                    if (with_exp)
                        exp_tab_vec(acc[i], tab, eg);
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (s < n_seed) {
                            const ConstF64 sfk = (ConstF64) (unsigned long long) Z->tabs.fk[s];
                            double Iv[VEC];
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                Iv[v] = f0[s][i] * sfk[kb + v];
                            if (with_exp) {
#pragma unroll
                                for (int v = 0; v < VEC; v++)
                                    Iv[v] *= eg[v];
                            }
#pragma unroll
                            for (int v = 0; v < VEC; v++) {
                                neg |= Iv[v] < 0.0 ? 1u << (s * LCH + i) : 0u; // (min over k of Iv negative, NaNs ignored: error -2, Helper.h:582-594)
                                angsum[s][i] += dv2[kb + v] * Iv[v];           // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                            }
                            if (!safe_check) { // the checking pass of a failing run integrates without depositing
                                // E_v of (s, n): the wave sum over the lanes that deposit into that record, into its accumulator
                                const bool dep = has_pix && ((live >> (s * LCH + i)) & 1u) != 0u;
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX (s * L + L - 1 - (a0 + i)) * Kp + kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
                            }
                        }
                    }
                }
            }
        }
        // ---- per (seed, record) of the chunk: the failure test (Helper.h:582-594), the I_ang add, the segmented nf scan ----
#pragma unroll
        for (int i = 0; i < LCH; i++) {
            if (a0 + i < L) {
                const int jb = L - 1 - (a0 + i); // block (within a seed's curve) and bit of this n
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
                        const bool lv      = ((live >> (s * LCH + i)) & 1u) != 0u;
                        const bool bad_neg = ((neg >> (s * LCH + i)) & 1u) != 0u, bad_nan = angsum[s][i] != angsum[s][i];
                        const bool failing = bad_neg || bad_nan;
                        if (lv && failing && !safe_skip) {
                            const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                            code |= c;
                            atomicOr(&H.ctl->seed_len_code[s][jb], c);
                            if (safe_check) // the lane that holds the ray writes its bits, chunk by chunk
                                bad64[ridx] |= 1ull << (32 * s + jb);
                        }
                        if (!safe_check) {
                            double *blk = Q->out + (size_t) (s * L + jb) * (size_t) Q->stride;
                            // a ray that fails under (s, n) adds nothing to that record (RayTraceImageCPU.cpp:29-36)
                            if (ang >= 0 && lv && !failing) {
                                if (lds_iang)
                                    unsafeAtomicAdd(&lds_iang[(s * L + jb) * seeds_ang_stride(H.n_ang) + ang], angsum[s][i]);
                                else
                                    unsafeAtomicAdd(&blk[Q->ang_off + (unsigned) ang], angsum[s][i]);
                            }
                            // nf: the segmented scan over the runs of equal pixel of the tile (rt_wave_runscan.inc), one atomic per run tail
                            double a = (has_pix && lv && !failing) ? angsum[s][i] * H.scale : 0.0;
#include "rt_wave_runscan.inc"
                            if (tail && a != 0.0)
                                unsafeAtomicAdd(&blk[Q->nf_off + (unsigned) pix], a);
                        }
                    }
                }
            }
        }
    }
    if (code) // one report per ray, whatever the number of seeds and n it fails under
        report_failure(code);
}

// The shell of rt_step_scan_seeds_kernel, word for word: one record per (seed, n), per record an I_ang histogram,
// seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.  The launch bounds of rt_step_rscan_kernel<false>.
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_step_rscan_seeds_kernel(const ScanSeedsKArg A)
{
    const FreqHot &H = A.hot;
#define STEP_WG_NREC A.set.n_seed * H.L
#define STEP_WG_ANG_STRIDE seeds_ang_stride(n_ang)
#define STEP_WG_ANG_ZERO n_rec * ang_stride
#define STEP_WG_RECORD(r) double *blk = A.scan.out + (size_t) r * (size_t) A.scan.stride;
#define STEP_WG_EV(r, c) blk[c]
#define STEP_WG_IANG(r, c) blk[A.scan.ang_off + c]
#define STEP_WG_PROLOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_PROLOGUE
    const int lane = lane_id();
    // the cold half, the scan block and the seeds of the argument block, the flag word and the lane number opaque per tile
#define HANDOUT_TILES_PER_FETCH FREQ_TILES_PER_FETCH_GAIN
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C    = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanSeedsKArg, cold));     \
    ScanPtr Q    = (ScanPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanSeedsKArg, scan));     \
    ScanSetPtr Z = (ScanSetPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanSeedsKArg, set));   \
    asm volatile("" : "+s"(C), "+s"(Q), "+s"(Z));                                                                                      \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    int n_seed_t    = A.set.n_seed;                                                                                                    \
    asm volatile("" : "+s"(hflags), "+v"(lane_t), "+s"(n_seed_t));                                                                     \
    step_rscan_seeds_tile(H, hflags, C, Q, Z, n_seed_t, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
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
