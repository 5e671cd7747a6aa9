#pragma once
// rt_step_scan_ase_seeds.hip -- step mode of an EMISSION plan with a length scan AND ASE seeds of the scan
// (rt_hip_plan_set_scan_ase_seeds): the whole per-step record -- the ASE triple and one seeded triple per seed beam -- at
// every plasma length n = 2 .. N from ONE forward march.
//
// The two premises are those of rt_step_ase_seeds.hip and rt_step_scan.hip: the march does not depend on the emission
// switch apart from evl, and the forward run of n lengths is a prefix of the run of N.  The march is the scan march
// unchanged (MODE 3, MARCH_OPT_SCAN); rt_step_scan_ase_seeds_kernel stands where rt_step_scan_kernel stands and leaves
// (1 + n_seed) L records, record (r, j) = block r L + (j - 1) -- a record's curve is contiguous, the ASE curve first:
//   (0, j)       what rt_step_scan_kernel<true> leaves for length j on this plan: the per-slot SF = 0 emission text
//                (ase_step / ase_update, wnan, exact emission honoured), the plan's scale
//   (1 + s, j)   what rt_step_scan_seeds_kernel leaves for (s, j) on a plan of the same problem created with a seed:
//                gain-only, Iv[k] = (f0_s sfk_s[k]) eg_j[k], one exp_tab_vec per length for all seeds, scale scales[s]
// The shell is that of every step pass (rt_step_wg.inc, rt_step_handout.inc), rt_tile_ray.inc / rt_tile_rec.inc with
// SF = 0, the boundary states and the table "which state serves length j" of rt_step_scan.hip -- one place_ray per length,
// shared by all records --, the per-seed factor at the launch ray of rt_step_scan_seeds.hip (on a forward ray grid the
// product of the seed's tabulated factors, otherwise scan_seed_factor; 0 where the ray has escaped by that length).
//
// Per tile the lengths are taken in chunks of SCAN_ASE_LCH = 2, and per chunk the frequencies are walked TWICE, as the
// SF = 6 instance of rt_step_ase_seeds_kernel does (its HALVES): first the emission recurrence over the slots with the sum
// of record (0, j) per length, then the f64 product sum gl with the sums of (1 + s, j).  One loop with both would hold the
// running Iv, wnan and gl of a batch beside 1 + n_seed sums per length; in two loops the emission half holds two sums and
// the two launch factors, the seed half six sums: 115 VGPRs, no scratch, four waves per SIMD.  Larger chunks spill; four
// lengths for the emission half with two and two for the seed half fit by registers (126) and keep a 48-byte stack frame
// (profiles/scan_ase_seeds_kernel_resources.txt has the alternatives).
// Both halves start at slot 0 per chunk and batch: the slots below the chunk are integrated again without depositing.
// At the end of a chunk, per length: the runs of equal pixel once (rt_wave_runs.inc), then per record the failure test,
// the I_ang add and the segmented nf scan (rt_wave_runscan.inc).  Everything per (record, length) is a register under
// wave-uniform unrolled tests.
//
// F_SKIP (rt_step_ase_seeds.hip): a ray whose sums over the whole N-run are all zero is masked from the ASE records only
// and is live for the seed records; a tile none of whose rays is live for record 0 skips the emission half.  A ray whose
// sums are zero up to some length only is not marked: it adds +0 to the shorter ASE records by arithmetic.
//
// Failures follow the reference run once per (record, length): error -1 at length j puts the ray in no record of that
// length and sets bit 1 in the code of every (r, j); error -2 / -3 under (r, j) removes the ray from (r, j) only.  A failing
// ray is reported once, with the OR of its codes; DevCtl::rec_len_code[r][j - 1] holds the code of (r, j).  The checking
// repeat keeps its two passes; the mark of a ray is one bit per (record, length), bit j - 1 of word r of four 32-bit words
// per ray (FreqHot::bad is an array of such 16-byte marks here), written by the one lane that holds the ray.
#include "rt_step_scan_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

constexpr int SCAN_ASE_LCH = 2; // lengths per pass over a tile
static_assert(1 + RT_N_SEED_MAX <= 4 && RT_N_SCAN_MAX <= 32, "one mark bit per (record, length) in four 32-bit words per ray");

// the seeds and the scales of the records: what rt_step_scan_ase_seeds_kernel reads beside the blocks of rt_step_scan_kernel
// (through the constant address space, where it is needed)
struct ScanAseSeedsArg {
    int n_seed;
    int pad;
    double scale[1 + RT_N_SEED_MAX]; // of every record's curve (scale[0] is the plan's, FreqHot::scale)
    SeedTabs tabs;
};
static_assert(offsetof(ScanAseSeedsArg, tabs) == 8 + sizeof(double) * (1 + RT_N_SEED_MAX) &&
                  sizeof(ScanAseSeedsArg) == offsetof(ScanAseSeedsArg, tabs) + sizeof(SeedTabs),
              "nesting SeedTabs moves no byte of the argument block");
struct ScanAseSeedsKArg {
    FreqHot hot;
    FreqCold cold;
    ScanArg scan; // out: (1 + n_seed) L blocks, block r L + (j - 1) the record of r (0: ASE, 1 + s: seed s) at length j
    ScanAseSeedsArg set;
};
typedef const RT_CONST_AS ScanAseSeedsArg *ScanAsePtr;

__device__ __forceinline__ void step_scan_ase_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, ScanPtr Q, ScanAsePtr Z, const int n_seed,
                                                         double *lds_iang, double *lds_ev, const double *tab, double *xpose, const unsigned tile,
                                                         const int lane)
{
    constexpr int SF      = 0; // (the text fragments below read it: slots at run time)
    constexpr int LCH     = SCAN_ASE_LCH;
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
    unsigned *bad32       = reinterpret_cast<unsigned *>(H.bad); // four words per ray: word r the lengths of record r

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
    // per seed: the seed factor at the launch ray, place_ray's arithmetic and order (Helper.h:523-533), as
    // step_scan_seeds_tile computes it; the tables of the seeds exist on a forward ray grid, for all seeds or none
    double f0_launch[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        f0_launch[s] = 0.0;
    if (have) {
        if (!Z->tabs.sf[0]) {
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
    (void) gv_nan; // (SF = 0 tests every frequency's lineshape values as it reads them)
    const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;

    unsigned code = 0u; // OR of this ray's codes over records and lengths

    for (int j0 = 0; j0 < L; j0 += LCH) {
        int pix[LCH], ang[LCH];
        double angsum[1 + NS][LCH];
        // bit li: the ray is placed at / carries its seed factors at length j0 + li + 1; bit r LCH + li: the ray is live under /
        // has had a negative Iv under record r at that length
        unsigned placed = 0u, seeded = 0u, live = 0u, neg = 0u;
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            const int j = j0 + li + 1; // the length, 1-based
            pix[li]     = -1;
            ang[li]     = -1;
#pragma unroll
            for (int r = 0; r < 1 + NS; r++)
                angsum[r][li] = 0.0;
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
                if (e1 && !safe_skip) { // error -1 at this length, whatever the record: reported (once, below), out of every record (r, j)
                    code |= 1u << 1;
#pragma unroll
                    for (int r = 0; r < 1 + NS; r++)
                        if (r <= n_seed)
                            atomicOr(&H.ctl->rec_len_code[r][j - 1], 1u << 1);
                }
                if (have && !e1) {
                    // pixel and angle cell of the exit state (the probe's exit ray is that of the whole run: j == L)
                    const unsigned pf = (hflags & ~(unsigned) (FQ_HAS_SEED | FQ_PROBE)) | (j == L ? (hflags & (unsigned) FQ_PROBE) : 0u);
                    const Placed P    = place_ray(pf, C, R, H.nx, backward, ridx, mj, flj, ray);
                    placed |= 1u << li;
                    pix[li] = P.pix;
                    ang[li] = P.ang;
                    if (!(flj & F_ESCAPED)) // (an escaped ray's seed factor is 0, Helper.h:523-533)
                        seeded |= 1u << li;
                    // live under record r: not where the checking pass found the ray failing; record 0: not a ray the march
                    // marked F_SKIP (the seed records take it)
#pragma unroll
                    for (int r = 0; r < 1 + NS; r++) {
                        if (r <= n_seed) {
                            const unsigned marked = safe_skip ? bad32[4u * ridx + (unsigned) r] : 0u;
                            if (!((marked >> (j - 1)) & 1u) && !(r == 0 && (fl & F_SKIP)))
                                live |= 1u << (r * LCH + li);
                        }
                    }
                }
            }
            // (one placement after the other, as in rt_step_scan.hip)
            asm volatile("" ::: "memory");
        }
        if (__ballot(placed != 0u) == 0ull)
            continue;
        constexpr unsigned chunk_bits = (1u << LCH) - 1u;
        const bool any0               = __ballot((live & chunk_bits) != 0u) != 0ull; // (else rt_step_scan_kernel skips the chunk)

        const int s_lo = j0 * RT_N_SUB; // the slots below the chunk: integrated again, nothing deposited
        // ---- the emission half: records (0, j) of the chunk, the EMIS text of step_scan_tile ----
        if (any0) {
            for (int kb = 0; kb < K; kb += VEC) {
                double acc[VEC]; // the running Iv
                bool wnan[VEC];  // a NaN or infinity among this frequency's lineshape values so far (0 * NaN on the CPU)
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    acc[v]  = 0.0;
                    wnan[v] = false;
                }
                // one sub-segment: the SF = 0 text of rt_tile_batch.inc
                auto slot_step = [&](int s) {
                    asm volatile("" : "+s"(s)); // (opaque, as in rt_step_scan.hip)
                    const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
                    const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                    const FVec w     = *reinterpret_cast<const FVec *>(row);
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
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            Iv[v] = wnan[v] ? __builtin_nan("") : acc[v];
#pragma unroll
                        for (int v = 0; v < VEC; v++) {
                            neg |= Iv[v] < 0.0 ? 1u << li : 0u; // (min over k of Iv negative, NaNs ignored: error -2, Helper.h:582-594)
                            angsum[0][li] += dv2[kb + v] * Iv[v]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                        }
                        if (!safe_check) { // the checking pass of a failing run integrates without depositing
                            const bool dep = pix[li] >= 0 && ((live >> li) & 1u) != 0u;
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX (j0 + li) * Kp + kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
                        }
                    }
                }
            }
        }
        // ---- the seed half: records (1 + s, j) of the chunk, the text of step_scan_seeds_tile ----
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
                                neg |= Iv[v] < 0.0 ? 1u << ((1 + s) * LCH + li) : 0u; // (error -2, Helper.h:582-594)
                                angsum[1 + s][li] += dv2[kb + v] * Iv[v];             // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                            }
                            if (!safe_check) {
                                // E_v of (1 + s, j): the wave sum over the lanes that deposit into that record, its scale, its accumulator
                                const bool dep       = pix[li] >= 0 && ((live >> ((1 + s) * LCH + li)) & 1u) != 0u;
                                const double scale_s = Z->scale[1 + s];
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX ((1 + s) * L + j0 + li) * Kp + kb
#define EV_SUM_SCALE scale_s
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
#undef EV_SUM_SCALE
                            }
                        }
                    }
                }
            }
        }
        // ---- per length of the chunk: the runs of equal pixel once; per record the failure test (Helper.h:582-594), the
        // I_ang add and the segmented nf scan ----
#pragma unroll
        for (int li = 0; li < LCH; li++) {
            if (j0 + li < L) {
                const int jb  = j0 + li; // block (within a record's curve) and bit of this length
                const int px  = pix[li];
                const bool dp = px >= 0;
                unsigned failing = 0u; // bit r: the ray fails under record r at this length
#pragma unroll
                for (int r = 0; r < 1 + NS; r++) {
                    if (r <= n_seed) {
                        const bool bad_neg = ((neg >> (r * LCH + li)) & 1u) != 0u, bad_nan = angsum[r][li] != angsum[r][li];
                        if (bad_neg || bad_nan) {
                            failing |= 1u << r;
                            if (((live >> (r * LCH + li)) & 1u) && !safe_skip) {
                                const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                                code |= c;
                                atomicOr(&H.ctl->rec_len_code[r][jb], c);
                                if (safe_check) // the lane that holds the ray writes its bits, chunk by chunk (a chunk's lengths are its own)
                                    bad32[4u * ridx + (unsigned) r] |= 1u << jb;
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
                    for (int r = 0; r < 1 + NS; r++) {
                        if (r <= n_seed) {
                            // a ray that fails under (r, j) adds nothing to that record (RayTraceImageCPU.cpp:29-36)
                            const bool ok = ((live >> (r * LCH + li)) & 1u) && !((failing >> r) & 1u);
                            double *blk   = Q->out + (size_t) (r * L + jb) * (size_t) Q->stride;
                            if (ang[li] >= 0 && ok) {
                                if (lds_iang)
                                    unsafeAtomicAdd(&lds_iang[(r * L + jb) * seeds_ang_stride(H.n_ang) + ang[li]], angsum[r][li]);
                                else
                                    unsafeAtomicAdd(&blk[Q->ang_off + (unsigned) ang[li]], angsum[r][li]);
                            }
                            double a = (dp && ok) ? angsum[r][li] * (r == 0 ? H.scale : Z->scale[r]) : 0.0;
#include "rt_wave_runscan.inc"
                            if (tail && a != 0.0)
                                unsafeAtomicAdd(&blk[Q->nf_off + (unsigned) px], a);
                        }
                    }
                }
            }
        }
    }
    if (code) // one report per ray, whatever the number of records and lengths it fails at
        report_failure(code);
}

// The shell of rt_step_kernel (rt_step_wg.inc, rt_step_handout.inc) with one record per (record of the step, length): per
// record an I_ang histogram, seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.  The register budget of
// rt_step_scan_kernel<true>.
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES) rt_step_scan_ase_seeds_kernel(const ScanAseSeedsKArg A)
{
    const FreqHot &H = A.hot;
#define STEP_WG_NREC (1 + A.set.n_seed) * H.L
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
#define HANDOUT_TILES_PER_FETCH FREQ_TILES_PER_FETCH_EMIS
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C    = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanAseSeedsKArg, cold));  \
    ScanPtr Q    = (ScanPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanAseSeedsKArg, scan));  \
    ScanAsePtr Z = (ScanAsePtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(ScanAseSeedsKArg, set)); \
    asm volatile("" : "+s"(C), "+s"(Q), "+s"(Z));                                                                                      \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    int n_seed_t    = A.set.n_seed;                                                                                                    \
    asm volatile("" : "+s"(hflags), "+v"(lane_t), "+s"(n_seed_t));                                                                     \
    step_scan_ase_seeds_tile(H, hflags, C, Q, Z, n_seed_t, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
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
