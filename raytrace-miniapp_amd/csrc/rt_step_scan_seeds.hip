#pragma once
// rt_step_scan_seeds.hip -- step mode with a length scan AND the seeds of the scan (rt_hip_plan_set_scan_seeds): the step
// record of every seed beam s < n_seed <= RT_N_SEED_MAX at every plasma length n = 2 .. N from ONE forward march.
//
// Neither the march nor the boundary states depend on the seed (rt_step_seeds.hip, rt_step_scan.hip say why): the seed enters
// as Iv[k] = f0_s f_s[4][k] exp(gl[k]) only, and exp(gl_j[k]) of length j is the same for every seed.  rt_step_scan_seeds_kernel
// stands where rt_step_scan_kernel stands, gain-only (an emission plan has no seed), and has its shape: the shell of
// rt_step_wg.inc / rt_step_handout.inc with n_rec = n_seed L records, record (s, j) = block s L + (j - 1) -- a seed's curve is
// contiguous --, rt_tile_ray.inc and rt_tile_rec.inc with SF = 0, the boundary states and the table "which state serves length
// j" of rt_step_scan.hip, the per-seed factor at the launch ray of rt_step_seeds.hip: on a forward ray grid the product of the
// seed's tabulated factors (RT_SEED_GRID_FACTOR), otherwise scan_seed_factor on the seed's DevSeed.
//
// Per frequency batch and length: gl and exp_tab_vec ONCE (needed if any seed's f0 != 0, or gl > 700, or gl is a NaN), then
// per seed Iv_s[v] = (f0_s sfk_s[kb + v]) eg[v] -- the association of both parent kernels, so every Iv_{s,j}[k] is the double a
// plain scan plan created with seed s computes --, the lane's sum over k and sign test of (s, j), and the E_v wave sum
// (rt_step_evsum.inc) into the accumulator of (s, j).  At the end of a chunk, per length: the runs of equal pixel once
// (rt_wave_runs.inc), then per seed the I_ang add and the segmented nf scan (rt_wave_runscan.inc).
//
// The lengths are taken in chunks of SCAN_SEEDS_LCH = 2 (rt_step_scan_kernel: 4): what is live per (seed, length) across the
// frequency loop is the sum over k, a double; RT_N_SEED_MAX x 2 of them are the four the plain scan kernel holds, with the
// second seed's launch factor in place of two of its four pixel / angle cells.  A chunk re-integrates the slots below it --
// 6 (c - 1) for chunk c, a product sum per slot in this mode, no exponential.  Seed and length loops are unrolled under
// wave-uniform tests: nothing per (seed, length) is indexed memory.
//
// Failures follow the reference run once per seed and length: error -1 depends on neither -- s.z^2 < 0.01 of the state that
// serves length j sets bit 1 in the code of (s, j) for every s; error -2 / -3 under seed s at length j removes the ray from
// record (s, j) only.  A ray that fails anywhere is reported once, with the OR of its codes;
// DevCtl::seed_len_code[s][j - 1] holds the code of (s, j).  The checking repeat keeps its two passes; the mark of a ray is
// one bit per (seed, length), bit 32 s + (j - 1) of a 64-bit word per ray (FreqHot::bad is an array of such words here),
// written by the one lane that holds the ray.
#include "rt_step_scan.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int SCAN_SEEDS_LCH = 2; // lengths per pass over a tile
static_assert(RT_N_SEED_MAX * 32 <= 64 && RT_N_SCAN_MAX <= 32, "one mark bit per (seed, length) in a 64-bit word per ray");

// the seeds of a scan: what rt_step_scan_seeds_kernel reads beside the blocks of rt_step_scan_kernel (through the constant
// address space, where it is needed)
struct ScanSeedsArg {
    int n_seed;
    int pad;
    SeedTabs tabs;
};
static_assert(offsetof(ScanSeedsArg, tabs) == 8 && sizeof(ScanSeedsArg) == 8 + sizeof(SeedTabs), "nesting SeedTabs moves no byte of the argument block");
struct ScanSeedsKArg {
    FreqHot hot;
    FreqCold cold;
    ScanArg scan; // out: n_seed L blocks, block s L + (j - 1) the record of seed s at length j
    ScanSeedsArg set;
};
typedef const RT_CONST_AS ScanSeedsArg *ScanSetPtr;

__device__ __forceinline__ void step_scan_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, ScanSetPtr Z, const int n_seed,
                                                     double *lds_iang, double *lds_ev, const double *tab, double *xpose, const unsigned tile,
                                                     const int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH     = SCAN_SEEDS_LCH;
    constexpr int NS      = RT_N_SEED_MAX;
    const int L           = H.L;
    const int S           = L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned ridx   = tile * WAVE + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = false; // the forward method: the scan takes no other
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool safe_check = (hflags & FQ_SAFE_CHECK) != 0, safe_skip = (hflags & FQ_SAFE_SKIP) != 0;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;
    unsigned long long *bad64 = reinterpret_cast<unsigned long long *>(H.bad);

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
    // the segment the ray escaped in (never: L + 1)
    const int n_done = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
    const int e_seg  = (fl & F_ESCAPED) ? (n_done > 0 ? (n_done - 1) / RT_N_SUB + 1 : 1) : L + 1;
    // per seed: the seed factor at the launch ray, place_ray's arithmetic and order (Helper.h:523-533)
    double f0_launch[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        f0_launch[s] = 0.0;
    if (have) {
        if (!R.sf) {
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
            // the launch ray is a grid point: product of the seed's tabulated factors (RT_SEED_GRID_FACTOR)
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

    // the (seed, length) pairs under which the checking pass found this ray failing: it stays out of their records
    const unsigned long long marked = (safe_skip && have) ? bad64[ridx] : 0ull;
    unsigned code            = 0u;   // OR of this ray's codes over seeds and lengths
    unsigned long long marks = 0ull; // (seed, length) pairs (bit 32 s + j - 1) it fails at with -2 / -3

    for (int j0 = 0; j0 < L; j0 += LCH) {
        int pix[LCH], ang[LCH];
        double angsum[NS][LCH];
        // bit li: the ray is live at / carries its seed factors at length j0 + li + 1; bit s LCH + li: a negative Iv seen under
        // seed s at that length / the ray is marked under (s, that length)
        unsigned live = 0u, seeded = 0u, neg = 0u, out = 0u;
        bool any_live = false;
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            const int j = j0 + li + 1; // the length, 1-based
            pix[li]     = -1;
            ang[li]     = -1;
#pragma unroll
            for (int s = 0; s < NS; s++)
                angsum[s][li] = 0.0;
            if (j <= L) {
                // the state that serves length j (rt_step_scan.hip)
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
                if (e1 && !safe_skip) { // error -1 at this length, whatever the seed: reported (once, below), out of every record (s, j)
                    code |= 1u << 1;
#pragma unroll
                    for (int s = 0; s < NS; s++)
                        if (s < n_seed)
                            atomicOr(&H.ctl->seed_len_code[s][j - 1], 1u << 1);
                }
                if (have && !e1) {
                    // pixel and angle cell of the exit state (the probe's exit ray is that of the whole run: j == L)
                    const unsigned pf = (hflags & ~(unsigned) (FQ_HAS_SEED | FQ_PROBE)) | (j == L ? (hflags & (unsigned) FQ_PROBE) : 0u);
                    const Placed P    = place_ray(pf, C, R, H.nx, backward, ridx, mj, flj, ray);
                    if (!(fl & F_SKIP)) {
                        live |= 1u << li;
                        pix[li] = P.pix;
                        ang[li] = P.ang;
                        if (!(flj & F_ESCAPED)) // (an escaped ray's seed factor is 0, Helper.h:523-533)
                            seeded |= 1u << li;
#pragma unroll
                        for (int s = 0; s < NS; s++)
                            out |= ((marked >> (32 * s + j - 1)) & 1ull) ? 1u << (s * LCH + li) : 0u;
                    }
                }
                any_live = any_live || ((live >> li) & 1u);
            }
            // (one placement after the other, as in rt_step_scan.hip)
            asm volatile("" ::: "memory");
        }
        if (__ballot(any_live) == 0ull)
            continue;

        const int s_lo = j0 * RT_N_SUB; // the slots below the chunk: integrated again, nothing deposited
        for (int kb = 0; kb < K; kb += VEC) {
            double acc[VEC]; // the running gl
#pragma unroll
            for (int v = 0; v < VEC; v++)
                acc[v] = 0.0;
            // one sub-segment: the gain-only SF = 0 text of rt_tile_batch.inc
            auto slot_step = [&](int s) {
                asm volatile("" : "+s"(s)); // (opaque, as in rt_step_scan.hip)
                const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
                const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                const FVec w     = *reinterpret_cast<const FVec *>(row);
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[v] += (double) sl.g * (double) w.v[v];
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
                    // ---- the walk has reached length j0 + li + 1: exp(gl) once, then Iv per seed ----
                    const bool carries = ((seeded >> li) & 1u) != 0u;
                    bool need          = false;
#pragma unroll
                    for (int s = 0; s < NS; s++)
                        need = need || (carries && f0_launch[s] != 0.0);
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        need = need || acc[v] > 700.0 || acc[v] != acc[v];
                    const bool with_exp = __ballot(need) != 0ull;
                    double eg[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        eg[v] = 1.0;
                    if (with_exp)
                        exp_tab_vec(acc, tab, eg);
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (s < n_seed) {
                            const ConstF64 sfk = (ConstF64) (unsigned long long) Z->tabs.fk[s];
                            const double f0    = carries ? f0_launch[s] : 0.0;
                            double Iv[VEC];
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                Iv[v] = f0 * sfk[kb + v];
                            if (with_exp) {
#pragma unroll
                                for (int v = 0; v < VEC; v++)
                                    Iv[v] *= eg[v];
                            }
#pragma unroll
                            for (int v = 0; v < VEC; v++) {
                                neg |= Iv[v] < 0.0 ? 1u << (s * LCH + li) : 0u; // (min over k of Iv negative, NaNs ignored: error -2, Helper.h:582-594)
                                angsum[s][li] += dv2[kb + v] * Iv[v];            // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                            }
                            if (!safe_check) { // the checking pass of a failing run integrates without depositing
                                // E_v of (s, j): the wave sum over the lanes that deposit into that record, into its accumulator
                                const bool dep = pix[li] >= 0 && !((out >> (s * LCH + li)) & 1u);
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX (s * L + j0 + li) * Kp + kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
                            }
                        }
                    }
                }
            }
        }
        // ---- per length of the chunk: the runs of equal pixel once; per seed the failure test (Helper.h:582-594), the I_ang
        // add and the segmented nf scan ----
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            if (j0 + li < L) {
                const int jb  = j0 + li; // block (within a seed's curve) and bit of this length
                const int px  = pix[li];
                const bool dp = px >= 0;
                unsigned failing = 0u; // bit s: the ray fails under seed s at this length
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
                        const bool bad_neg = ((neg >> (s * LCH + li)) & 1u) != 0u, bad_nan = angsum[s][li] != angsum[s][li];
                        if (bad_neg || bad_nan) {
                            failing |= 1u << s;
                            if (((live >> li) & 1u) && !safe_skip) {
                                const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                                code |= c;
                                marks |= 1ull << (32 * s + jb);
                                atomicOr(&H.ctl->seed_len_code[s][jb], c);
                            }
                        }
                    }
                }
                if (!safe_check) {
#define RUNS_PIX px
#define RUNS_DEPOSITS dp
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        if (s < n_seed) {
                            // a ray that fails under (s, j) adds nothing to that record (RayTraceImageCPU.cpp:29-36)
                            const bool ok = !((failing >> s) & 1u) && !((out >> (s * LCH + li)) & 1u);
                            double *blk   = Q->out + (size_t) (s * L + jb) * (size_t) Q->stride;
                            if (ang[li] >= 0 && ok) {
                                if (lds_iang)
                                    unsafeAtomicAdd(&lds_iang[(s * L + jb) * seeds_ang_stride(H.n_ang) + ang[li]], angsum[s][li]);
                                else
                                    unsafeAtomicAdd(&blk[Q->ang_off + (unsigned) ang[li]], angsum[s][li]);
                            }
                            double a = (dp && ok) ? angsum[s][li] * H.scale : 0.0;
#include "rt_wave_runscan.inc"
                            if (tail && a != 0.0)
                                unsafeAtomicAdd(&blk[Q->nf_off + (unsigned) px], a);
                        }
                    }
                }
            }
        }
    }
    if (code) { // one report per ray, whatever the number of seeds and lengths it fails at
        report_failure(code);
        if (safe_check && marks)
            bad64[ridx] = marks; // the lane that holds the ray writes all its bits
    }
}

// The shell of rt_step_kernel (rt_step_wg.inc, rt_step_handout.inc) with one record per (seed, length): per record an I_ang
// histogram, seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_step_scan_seeds_kernel(const ScanSeedsKArg A)
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
    step_scan_seeds_tile(H, hflags, C, Q, Z, n_seed_t, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
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
