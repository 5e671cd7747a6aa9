#pragma once
// rt_spec_ase_seeds.hip -- spectra mode of an EMISSION plan that carries ASE seeds (rt_hip_plan_set_spectra_ase_seeds):
// RayTrace::calc_ray of the ASE problem AND of the same problem under up to RT_N_SEED_MAX seed beams, for every ray of a run,
// from ONE march and ONE pass over the march record.
//
// The premise is that of rt_step_ase_seeds.hip: the trajectory, gvl, the exit state, the escape flag and the step count do
// not depend on use_emis; only evl does.  The march record of an emission plan therefore holds everything the gain-only pass
// of a seeded run of the same problem reads, and rt_spec_ase_seeds_kernel<SF> leaves 1 + n_seed row blocks from it:
//   block 0       the row rt_spec_kernel<SF, true> leaves on this plan: the emission recurrence, the text of rt_tile_batch.inc
//                 over the decode of rt_tile_rec.inc with the mask spec_tile passes (have && !err1 && !F_SKIP), so the
//                 tile-wide choice is taken over the same lanes; exact emission and gv_nan included
//   block 1 + s   the row rt_spec_kernel<SF, false> leaves of the same problem created with seed s (E0 present and unused):
//                 gain-only, Iv[k] = (f0_s f_s[4][k]) exp(gl[k]), in the association and with the exponential-skip rule of
//                 rt_spec_seeds.hip (`need` over all seeds)
// It stands where rt_spec_kernel stands and has the shell of rt_spec_seeds_kernel: one 16-wave work-group per CU, tiles from
// the eight sharded counters, lanes = rays, the two exponent tables and ONE [64][XS_ROW] staging per wave in LDS.
//
// Per tile, once: the preamble (rt_tile_ray.inc), the -1 test, the exit ray, the probe, the record decode.  Then two halves
// over the frequencies, the HALVES of rt_step_ase_seeds.hip:
//   emission half  the loop of spec_tile<SF, true>: 16 values of 64 rows staged, 128-byte row segments into block 0
//   seed half      the loop of spec_seeds_tile<SF>: the seed factors first (forward at the launch ray -- on a ray grid the
//                  product of the seed's tabulated factors --, backward at the exit state; rscan_seed_factor on the seed
//                  where it lies in the argument block; taken here so that nothing of them is live across the emission loop),
//                  then the exponentials and f0_s staged, the storing lanes forming the products on the way out into blocks 1 + s
// The seed half reads the lineshape rows again, from the caches.  The narrow-group, ragged-tile and odd-K store paths are
// those of rt_spec.hip and rt_spec_seeds.hip.
//
// F_SKIP: the emission march marks a ray whose every gvl / evl sum is zero (never when a lineshape table holds a non-finite
// value, DevParams::no_skip).  It gets a row of zeros in block 0, as in rt_spec_kernel; under a seed it is live and carries
// f0_s f_s[4][k] exp(0).  Its zeroed slots and its real slots both give gl = +0 (its gs are all +0), so the one decode serves
// both halves.  A tile none of whose rays is live for block 0 skips the recurrence, writes block 0's zeros and runs the seed half.
//
// Outputs, block-major in the one allocation of the mode: Iv [1 + n_seed][n_rays][K] (row stride K), err [1 + n_seed][n_rays],
// ray2 [n_rays].  Error -1 and the exit ray do not depend on the block; -2 / -3 are per block, -2 wins.  Every element is written.
// Failures: a ray is reported once with the OR of its codes over the blocks; DevCtl::rec_code[r] carries the code of block r.
// Nothing is deposited: no checking repeat.
#include "rt_spec_seeds.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_spec.hip: the same contractions, the same doubles)

// the argument block is that of rt_spec_seeds_kernel: out holds 1 + n_seed blocks here
template <int SF>
__device__ __forceinline__ void spec_ase_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SpecSeedsPtr Q, const int n_seed, const double *tab,
                                                    double *stage, const unsigned tile, const int lane)
{
    constexpr int NS      = RT_N_SEED_MAX;
    constexpr bool EMIS   = true; // (rt_tile_batch.inc: block 0 is the emission text)
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

    // ---- per-ray preamble, once: record, -1 test, exit ray (Helper.h:514-521) ----
#define TILE_NEED_RAY false // (the seed half reads the launch ray where it needs it)
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    rt_ray r2 = { 0.0f, 0.0f, 0.0f, 0.0f }; // (the reference leaves ray2 untouched on error -1: zeros here)
    if (have && !err1) {
        r2.x = m.px; // Helper.h:518-521
        r2.y = m.py;
        r2.a = atanf_flt32_kernel(m.sx / m.sz) * 1e3f;
        r2.b = atanf_flt32_kernel(m.sy / m.sz) * 1e3f;
    }
    if (have) {
        Q->out.ray2[ridx] = r2;
        if (probe_on) {
            C->probe.ray2[ridx]  = r2;
            C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
            C->probe.steps[ridx] = steps;
        }
    }
    if (err1) { // error -1: reported once, and every block's code has the bit
        report_failure(1u << 1);
#pragma unroll
        for (int r = 0; r < 1 + NS; r++)
            if (r <= n_seed)
                atomicOr(&H.ctl->rec_code[r], 1u << 1);
    }
    // block 0: spec_tile's live mask -- a ray with error -1, and one whose every update is the identity (F_SKIP), gets a row
    // of zeros; the seed blocks: F_SKIP does not count
    const bool live     = have && !err1 && !(fl & F_SKIP);
    const bool any_live = __ballot(live) != 0ull;
    const bool lives    = have && !err1;

    // ---- the march record of this lane's ray, the slots of a lane without a ray live for block 0 zeroed (as spec_tile) ----
#define TILE_MASK live
#include "rt_tile_rec.inc"
#undef TILE_MASK
    // (the gain-only half of rt_tile_batch.inc is dead text here, EMIS is true: what it names)
    constexpr double f0 = 0.0;
    const ConstF64 sfk  = (ConstF64) (unsigned long long) H.seed_fk;

    // a full tile and an even K: every 16-frequency group that lies inside K leaves as 16-byte stores
    const bool wide_ok    = row0 + WAVE <= n_rays && (K & 1) == 0;
    const size_t blk_rows = (size_t) n_rays; // rows of one block
    unsigned code = 0u;

    // ================= the emission half: block 0, the loop of spec_tile<SF, true> =================
    {
        double *Iv0    = Q->out.Iv;
        double iv_min = 0.0;   // min over k of Iv, NaNs ignored: negative <=> error -2
        bool has_nan  = false; // error -3 unless -2 (Helper.h:588-593: negative wins)
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
                    double *dst        = Iv0 + ((size_t) (row0 + (unsigned) (lane >> 3)) * (size_t) K + (size_t) (kbase + 2 * (lane & 7)));
                    const size_t gstep = (size_t) 8 * (size_t) K; // eight rows on
                    const double *src  = stage + (lane >> 3) * XS_ROW + 2 * (lane & 7);
#pragma unroll 4
                    for (int g = 0; g < WAVE / 8; g++)
                        SPEC_STORE16(src + g * 8 * XS_ROW, dst + (size_t) g * gstep);
                } else if (wide_ok) {
                    // the last, narrower group of a row (2 .. 14 frequencies): 16 bytes per lane, the lanes dealt over the pieces
                    const unsigned hw = (unsigned) width >> 1; // 16-byte pieces per row
                    for (unsigned q = (unsigned) lane; q < WAVE * hw; q += WAVE) {
                        const unsigned row = q / hw, piece = q - row * hw;
                        SPEC_STORE16(stage + row * XS_ROW + 2 * piece, Iv0 + ((size_t) (row0 + row) * (size_t) K + (size_t) kbase + 2 * piece));
                    }
                } else {
                    // ragged tile or odd K: 8 bytes per lane, four rows per instruction
                    const int k = kbase + (lane & 15);
#pragma unroll 4
                    for (int g = 0; g < WAVE / 4; g++) {
                        const unsigned row = row0 + (unsigned) (4 * g + (lane >> 4));
                        if (row < n_rays && k < K)
                            Iv0[(size_t) row * (size_t) K + (size_t) k] = stage[(4 * g + (lane >> 4)) * XS_ROW + (lane & 15)];
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        const bool bad_neg = live && iv_min < 0.0, bad_nan = live && has_nan;
        if (have)
            Q->out.err[ridx] = err1 ? -1 : (bad_neg ? -2 : (bad_nan ? -3 : 0));
        if (bad_neg || bad_nan) {
            code = bad_neg ? (1u << 2) : (1u << 3);
            atomicOr(&H.ctl->rec_code[0], code);
        }
    }

    // ================= the seed half: blocks 1 + s, the loop of spec_seeds_tile<SF> =================
    // ---- per seed: the seed factor, place_ray's arithmetic and order (Helper.h:523-533), as spec_seeds_tile takes it: from
    // the record and the launch ray read again here ----
    double fs[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        fs[s] = 0.0;
    if (lives && !(fl & F_ESCAPED)) {
        const double *sf0 = Q->tabs.sf[0]; // (the tables of the seeds exist on a forward ray grid, for all seeds or none)
        if (backward || !sf0) {
            double px, py, pa, pb;
            if (backward) { // the exit state, Helper.h:518-521
                const RecMeta mm = *reinterpret_cast<const RecMeta *>(rec + rec_meta_off(rrec, S, H.rec_stride));
                px = (double) mm.px;
                py = (double) mm.py;
                pa = (double) (atanf_flt32_kernel(mm.sx / mm.sz) * 1e3f);
                pb = (double) (atanf_flt32_kernel(mm.sy / mm.sz) * 1e3f);
            } else { // the launch ray
                rt_ray lr = { 0, 0, 0, 0 };
                float ta, tb;
                load_ray(R, ridx, lr, ta, tb, false);
                px = (double) lr.x;
                py = (double) lr.y;
                pa = (double) lr.a;
                pb = (double) lr.b;
            }
            // (the seeds in a loop the compiler does not unroll, the factor filed by selects -- rt_spec_seeds.hip)
#pragma unroll 1
            for (int s = 0; s < n_seed; s++) {
                const double f = rscan_seed_factor(&Q->tabs.seed[s], px, py, pa, pb);
#pragma unroll
                for (int t = 0; t < NS; t++)
                    fs[t] = t == s ? f : fs[t];
            }
        } else {
            // the launch ray is a grid point: product of the seed's tabulated factors (RT_SEED_GRID_FACTOR)
            RT_SEED_GRID_POINT(R, ridx)
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const double *sf         = Q->tabs.sf[s];
                    const unsigned char *sin = Q->tabs.sin[s];
                    RT_SEED_GRID_FACTOR(fs[s], Q->tabs.seed[s].f0, sf, sin)
                }
            }
        }
    }
    const bool any_lives = __ballot(lives) != 0ull;
    // what the storing lanes need of a row beside its exponentials: whether it is live, and its seed factors -- once per tile
    // (the last flush of the emission half ended behind a wave barrier; the first flush of this half begins behind one)
    const unsigned long long live_mask = __ballot(lives);
#pragma unroll
    for (int s = 0; s < NS; s++)
        stage[lane * XS_ROW + SPEC_SEEDS_F0 + s] = fs[s];
    // (the gain sums opaque at the head of this half: (double) gs[s] is invariant in kb -- rt_step_ase_seeds.hip)
    float gq[SF ? SF : 1];
#pragma unroll
    for (int s = 0; s < (SF ? SF : 1); s++) {
        gq[s] = gs[s];
        asm volatile("" : "+v"(gq[s]));
    }

    double iv_min[NS]; // per seed: min over k of Iv, NaNs ignored: negative <=> error -2
    unsigned nanm = 0u; // bit s: a NaN among the values of seed s: error -3 unless -2
#pragma unroll
    for (int s = 0; s < NS; s++)
        iv_min[s] = 0.0;

    for (int kb = 0; kb < K; kb += VEC) {
        // gain only, Helper.h:569-580: f64 products summed in sub-segment order (the text of rt_tile_batch.inc); once
        double gl[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            gl[j] = 0.0;
        bool with_exp = false;
        if (any_lives) { // (else nothing to integrate: the rows are zeros)
            if (SF) {
                FVec w[SF ? SF : 1];
                load_rows(w, kb);
#pragma unroll
                for (int s = 0; s < SF; s++) {
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        gl[j] += (double) gq[s] * (double) w[s].v[j];
                }
            } else {
                for (int s = 0; s < S; s++) {
                    const RecSlot sl = rec_slot_lazy(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
                    const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
                    const FVec w     = *reinterpret_cast<const FVec *>(row);
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        gl[j] += (double) sl.g * (double) w.v[j];
                }
            }
            // Iv_s = f0_s f_s[4][k] exp(gl); for f0_s = 0 that is exactly 0 unless exp overflows (0 * inf): a wave none of whose
            // lanes needs the exponential under any seed skips it
            bool need = false;
#pragma unroll
            for (int s = 0; s < NS; s++)
                need = need || fs[s] != 0.0;
#pragma unroll
            for (int j = 0; j < VEC; j++)
                need = need || gl[j] > 700.0 || gl[j] != gl[j];
            with_exp = __ballot(need) != 0ull;
        }
        double eg[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            eg[j] = 1.0;
        if (with_exp)
            exp_tab_vec(gl, tab, eg);
        // ---- the exponentials into the lane's staging row; per seed the values of this lane for its scan (Helper.h:582-587) ----
        // (eg = 1 where the wave skipped the exponential: x * 1.0 is x, so the storing lanes need not know)
        double *mine = stage + lane * XS_ROW + (kb & 12);
#pragma unroll
        for (int j = 0; j < VEC; j++)
            mine[j] = eg[j];
        if (any_lives) {
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (s < n_seed) {
                    const ConstF64 sk = (ConstF64) (unsigned long long) Q->tabs.fk[s];
#pragma unroll
                    for (int j = 0; j < VEC; j++) {
                        const double v = (lives && kb + j < K) ? (fs[s] * sk[kb + j]) * eg[j] : 0.0; // (the padding columns K .. Kp-1 are not part of the spectrum)
                        iv_min[s]      = fmin(iv_min[s], v);
                        nanm |= v != v ? 1u << s : 0u;
                    }
                }
            }
        }
        if ((kb & 12) == 12 || kb + VEC >= K) {
            __builtin_amdgcn_wave_barrier();
            const int kbase = kb & ~15;
            const int width = K - kbase < 16 ? K - kbase : 16; // frequencies of this group
            // a value on its way out: (f0_s sfk_s[k]) eg of a live row, +0 of any other (a select: 0 * x would give NaN or -0)
            auto out2 = [&](const double *rowp, const int c, const int s, const bool lv, const f64x2s fk2) {
                const f64x2s e2 = *reinterpret_cast<const f64x2s *>(rowp + c);
                const double fr = rowp[SPEC_SEEDS_F0 + s];
                f64x2s r;
                r.x = lv ? (fr * fk2.x) * e2.x : 0.0;
                r.y = lv ? (fr * fk2.y) * e2.y : 0.0;
                return r;
            };
            if (wide_ok && width == 16) {
                // eight lanes cover the 128 bytes of a row, a store instruction eight rows, as in rt_spec.hip
                const int c = 2 * (lane & 7);
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double *fk = Q->tabs.fk[s] + kbase + c;
                    f64x2s fk2;
                    fk2.x       = fk[0];
                    fk2.y       = fk[1];
                    double *dst = Q->out.Iv + (size_t) (1 + s) * blk_rows * (size_t) K + ((size_t) (row0 + (unsigned) (lane >> 3)) * (size_t) K + (size_t) (kbase + c));
                    const size_t gstep = (size_t) 8 * (size_t) K; // eight rows on
#pragma unroll 4
                    for (int g = 0; g < WAVE / 8; g++) {
                        const int row      = 8 * g + (lane >> 3);
                        const double *srow = stage + row * XS_ROW;
                        const f64x2s r     = out2(srow, c, s, ((live_mask >> row) & 1ull) != 0ull, fk2);
                        *reinterpret_cast<f64x2s *>(dst + (size_t) g * gstep) = r;
                    }
                }
            } else if (wide_ok) {
                // the last, narrower group of a row (2 .. 14 frequencies): 16 bytes per lane, the lanes dealt over the pieces
                const unsigned hw = (unsigned) width >> 1; // 16-byte pieces per row
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double *fk = Q->tabs.fk[s] + kbase;
                    double *blk      = Q->out.Iv + (size_t) (1 + s) * blk_rows * (size_t) K;
                    for (unsigned q = (unsigned) lane; q < WAVE * hw; q += WAVE) {
                        const unsigned row = q / hw, piece = q - row * hw;
                        f64x2s fk2;
                        fk2.x          = fk[2 * piece];
                        fk2.y          = fk[2 * piece + 1];
                        const f64x2s r = out2(stage + row * XS_ROW, (int) (2 * piece), s, ((live_mask >> row) & 1ull) != 0ull, fk2);
                        *reinterpret_cast<f64x2s *>(blk + ((size_t) (row0 + row) * (size_t) K + (size_t) kbase + 2 * piece)) = r;
                    }
                }
            } else {
                // ragged tile or odd K: 8 bytes per lane, four rows per instruction
                const int k = kbase + (lane & 15);
#pragma unroll 1
                for (int s = 0; s < n_seed; s++) {
                    const double *fk = Q->tabs.fk[s];
                    double *blk      = Q->out.Iv + (size_t) (1 + s) * blk_rows * (size_t) K;
                    const double fkk = k < K ? fk[k] : 0.0;
#pragma unroll 4
                    for (int g = 0; g < WAVE / 4; g++) {
                        const int row = 4 * g + (lane >> 4);
                        if (row0 + (unsigned) row < n_rays && k < K) {
                            const double *srow = stage + row * XS_ROW;
                            const bool lv      = ((live_mask >> row) & 1ull) != 0ull;
                            blk[(size_t) (row0 + (unsigned) row) * (size_t) K + (size_t) k] = lv ? (srow[SPEC_SEEDS_F0 + s] * fkk) * srow[lane & 15] : 0.0;
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    // ---- the codes per seed block: -1 of the ray, else -2 over -3; a failing ray is reported once, with the codes of all blocks ----
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            const bool bad_neg = lives && iv_min[s] < 0.0, bad_nan = lives && ((nanm >> s) & 1u) != 0u;
            if (have)
                Q->out.err[(size_t) (1 + s) * blk_rows + ridx] = err1 ? -1 : (bad_neg ? -2 : (bad_nan ? -3 : 0));
            if (bad_neg || bad_nan) {
                const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                code |= c;
                atomicOr(&H.ctl->rec_code[1 + s], c);
            }
        }
    }
    if (code)
        report_failure(code);
}

// The shell of rt_spec_seeds_kernel (and its argument block): one work-group of FREQ_WG_WAVES waves per CU, tiles from the eight
// sharded counters, one tile per fetch; LDS, all dynamic: the two exponent tables, then [64][XS_ROW] staging doubles per wave.
// The register budget of rt_spec_kernel<SF, true>.
template <int SF>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES) rt_spec_ase_seeds_kernel(const SpecSeedsKArg A)
{
    const int n_seed = A.set.n_seed;
    // per tile: the cold half and the seeds of the argument block, the flag word and the lane number opaque
#define SPEC_WG_KERNEL
#define SPEC_WG_TILE                                                                                                    \
    ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecSeedsKArg, cold)); \
    SpecSeedsPtr Q = (SpecSeedsPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SpecSeedsKArg, set)); \
    asm volatile("" : "+s"(C), "+s"(Q)); \
    unsigned hflags = H.flags; \
    int lane_t      = lane; \
    asm volatile("" : "+s"(hflags), "+v"(lane_t)); \
    spec_ase_seeds_tile<SF>(H, hflags, C, Q, n_seed, exp2_tab, stage, tile, lane_t);
#include "rt_spec_wg.inc"
#undef SPEC_WG_TILE
#undef SPEC_WG_KERNEL
}

} // namespace rt
