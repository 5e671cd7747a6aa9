#pragma once
// rt_step_seeds.hip -- step mode with a seed set (rt_hip_plan_set_seeds): the records of up to RT_N_SEED_MAX seed beams
// from ONE march.
//
// The application's per-step record (intensity_step_struct, src/RayTraceStructures.h:361-369) holds one seeded triple
// E_v_seed[s], image_seed[s], E_ang_seed[s] per seed beam, s < N_seed <= N_SEED_MAX = 2.  The march record (gvl / evl /
// ivl, exit point, direction, flags) holds nothing of the seed (Helper.h:428-521): the seed enters in the frequency pass
// only, as Iv[k] = f0_s f_s[4][k] exp(gl[k]) (Helper.h:523-533, 569-580), and exp(gl[k]) is the same for every seed.
// rt_step_seeds_kernel stands where rt_step_kernel stands, gain-only, and has its shape: one 16-wave work-group per CU,
// tiles from the eight sharded counters, lanes = rays; the per-ray preamble (rt_tile_ray.inc) and the record decode
// (rt_tile_rec.inc) are the text rt_step.hip includes.  Per tile, once: preamble, decode, pixel and angle cell (place_ray
// without its seed half).  Per seed: f0_s in place_ray's own arithmetic and order -- on a forward ray grid the product of
// the seed's tabulated factors with the clamp, otherwise seed_factor on the seed's DevSeed.  Per frequency batch: gl[] and
// exp_tab_vec once (needed if any seed's f0 != 0, or gl > 700, or gl is a NaN), then per seed in turn
// Iv_s[j] = (f0_s sfk_s[kb + j]) eg[j] -- the double rt_step_kernel computes for that seed, in its association -- the lane's
// sums and the E_v wave sum into the seed's accumulator in LDS; only f0_s, angsum_s and iv_min_s are live per seed.
// Per tile end and seed: the I_ang add and the segmented nf scan of rt_step.hip (the runs of equal pixel are found once).
//
// Failures follow the reference run once per seed: error -1 does not depend on the seed (the ray deposits into no record,
// every seed's code carries the bit); error -2 / -3 under seed s removes the ray from record s only
// (RayTraceImageCPU.cpp:29-36 per create_image call).  The checking repeat (plan_repeat_checked) keeps its two passes; the
// mark of a ray in bad[] is one bit per seed, written by the one lane that holds the ray.  A ray that fails under any seed
// is reported once, with the OR of its codes, into the control block; DevCtl::seed_code[s] holds the code of seed s.
#include "rt_step.hip"

namespace rt {

#pragma clang fp contract(fast) // (the float64 half, as in rt_freq.hip and rt_step.hip: the same contractions, the same doubles)

// the record of one seed: E_v [K], nf [nx * ny], I_ang [na * nb] inside the plan's one allocation
struct SeedRec {
    double *E_v, *nf, *iang;
};
// what rt_step_seeds_kernel reads beside the frequency kernel's block: read through the constant address space where it
// is needed (as the cold half is), so that nothing of it is live across the frequency loop
struct SeedSetArg {
    int n_seed;
    int pad;
    SeedRec out[RT_N_SEED_MAX];
    const double *fk[RT_N_SEED_MAX];         // [Kp] f[4] of the seed, zero padded
    const double *sf[RT_N_SEED_MAX];         // forward ray grid: the seed's factor tables (rt_seed_tab_kernel), else NULL
    const unsigned char *sin[RT_N_SEED_MAX]; // ... and its support flags
    DevSeed seed[RT_N_SEED_MAX];
};
struct SeedsKArg {
    FreqHot hot;
    FreqCold cold;
    SeedSetArg set;
};
typedef const RT_CONST_AS SeedSetArg *SetPtr;

// doubles from one seed's I_ang histogram in LDS to the next: na * nb and two cells to spare (on an axis of one grid point
// the angle cell of a ray can be one past the grid, see rt_hip_plan_run; such a cell must not be the next seed's), even
__host__ __device__ constexpr int seeds_ang_stride(int n_ang) { return (n_ang + 3) & ~1; }
// doubles of dynamic LDS of a work-group (layout: rt_step_seeds_kernel)
inline size_t step_seeds_lds_doubles(bool iang_in_lds, int n_ang, int Kp, int wg_waves, int n_seed)
{
    return (size_t) 2 * EXP_TAB + (size_t) n_seed * ((iang_in_lds ? (size_t) seeds_ang_stride(n_ang) : 0) + (size_t) Kp) + (size_t) wg_waves * (size_t) (4 * XP_ROW);
}

template <int SF>
__device__ __forceinline__ void step_seeds_tile(const FreqHot &H, const unsigned hflags, ColdPtr C, SetPtr Q, const int n_seed, double *lds_iang,
                                                double *lds_ev, const double *tab, double *xpose, const unsigned tile, const int lane)
{
    constexpr int NS      = RT_N_SEED_MAX;
    const int S           = SF ? SF : H.L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned ridx   = tile * WAVE + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = H.method == 1;
    const unsigned rrec      = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool safe_check = (hflags & FQ_SAFE_CHECK) != 0, safe_skip = (hflags & FQ_SAFE_SKIP) != 0;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;

    // ---- per-ray preamble, once: exit ray, deposit cells (rt_tile_ray.inc, place_ray without its seed half) ----
#define TILE_NEED_RAY (!(hflags & FQ_OWN_CELLS) || probe_on)
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    double f0[NS];
#pragma unroll
    for (int s = 0; s < NS; s++)
        f0[s] = 0.0;
    int pix = -1, ang = -1;
    if (have && !err1) {
        const Placed P = place_ray(hflags & ~(unsigned) FQ_HAS_SEED, C, R, H.nx, backward, ridx, m, fl, ray);
        pix = P.pix;
        ang = P.ang;
        // ---- per seed: the seed factor, place_ray's arithmetic and order (Helper.h:523-533) ----
        if (!(fl & F_ESCAPED)) {
            if (backward || !R.sf) {
                float ra = 0.0f, rb = 0.0f;
                if (backward) { // Helper.h:518-521: atanf(s.x / s.z) * 1e3f
                    ra = atanf_flt32_kernel(m.sx / m.sz) * 1e3f;
                    rb = atanf_flt32_kernel(m.sy / m.sz) * 1e3f;
                }
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
                        const DevSeed SD = load_cold(&Q->seed[s]);
                        f0[s] = backward ? seed_factor(SD, (double) m.px, (double) m.py, (double) ra, (double) rb)
                                         : seed_factor(SD, (double) ray.x, (double) ray.y, (double) ray.a, (double) ray.b);
                    }
                }
            } else {
                // the launch ray is a grid point: product of the seed's tabulated factors, in seed_factor's order
                unsigned gi, gj, gk, gm;
                grid_index(R, ridx, gi, gj, gk, gm);
                const unsigned oj = (unsigned) R.ngx, ok = oj + (unsigned) R.ngy, om = ok + (unsigned) R.nga;
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (s < n_seed) {
                        const double *sf         = Q->sf[s];
                        const unsigned char *sin = Q->sin[s];
                        if (sin[gi] & sin[oj + gj] & sin[ok + gk] & sin[om + gm]) {
                            const double v = Q->seed[s].f0 * sf[gi] * sf[oj + gj] * sf[ok + gk] * sf[om + gm];
                            f0[s]          = v < 0.0 ? 0.0 : v;
                        }
                    }
                }
            }
        }
    }
    if (have && probe_on) {
        C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
        C->probe.steps[ridx] = steps;
    }
    if (err1 && !safe_skip) { // error -1: the ray is reported (once), deposits into no record, and every seed's code has the bit
        report_failure(1u << 1);
#pragma unroll
        for (int s = 0; s < NS; s++)
            if (s < n_seed)
                atomicOr(&H.ctl->seed_code[s], 1u << 1);
    }
    const unsigned all_seeds = (1u << n_seed) - 1u;
    // the seeds under which the checking pass found this ray failing: it stays out of their records
    const unsigned marked = (safe_skip && have) ? ((unsigned) H.bad[ridx] & all_seeds) : 0u;
    const bool live       = have && !err1 && !(fl & F_SKIP) && marked != all_seeds;
    if (__ballot(live) == 0ull)
        return;
    if (!live) {
        pix = -1;
        ang = -1;
    }

    // ---- the march record of this lane's ray and the tile-wide choice of the update, once (rt_tile_rec.inc) ----
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
    (void) rs;
    (void) all_small;
    (void) gv_nan;
    const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;

    double angsum[NS], iv_min[NS]; // per seed: RayTraceImageCPU.cpp:63-68 sequential in k, and min over k of Iv (Helper.h:582-594)
#pragma unroll
    for (int s = 0; s < NS; s++) {
        angsum[s] = 0.0;
        iv_min[s] = 0.0;
    }
    const bool dep = pix >= 0; // this lane's ray deposits into the images of the seeds it is not marked under

    for (int kb = 0; kb < K; kb += VEC) {
        // gain only, Helper.h:569-580: f64 products summed in sub-segment order (the text of rt_tile_batch.inc); once
        double gl[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            gl[j] = 0.0;
        if (SF) {
            FVec w[SF ? SF : 1];
            load_rows(w, kb);
#pragma unroll
            for (int s = 0; s < SF; s++) {
#pragma unroll
                for (int j = 0; j < VEC; j++)
                    gl[j] += (double) gs[s] * (double) w[s].v[j];
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
            need = need || f0[s] != 0.0;
#pragma unroll
        for (int j = 0; j < VEC; j++)
            need = need || gl[j] > 700.0 || gl[j] != gl[j];
        const bool with_exp = __ballot(need) != 0ull;
        double eg[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++)
            eg[j] = 1.0;
        if (with_exp)
            exp_tab_vec(gl, tab, eg);
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (s < n_seed) {
                const ConstF64 sfk = (ConstF64) (unsigned long long) Q->fk[s];
                double Iv[VEC];
#pragma unroll
                for (int j = 0; j < VEC; j++)
                    Iv[j] = f0[s] * sfk[kb + j];
                if (with_exp) {
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        Iv[j] *= eg[j];
                }
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    iv_min[s] = fmin(iv_min[s], Iv[j]);
                    angsum[s] += dv2[kb + j] * Iv[j]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
                }
                if (!safe_check) { // the checking pass of a failing run integrates without depositing
                    // E_v of seed s: the wave sum of rt_step.hip over the lanes that deposit under this seed
                    const bool dep_s = dep && !((marked >> s) & 1u);
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        xpose[j * XP_ROW + lane] = dep_s ? Iv[j] : 0.0;
                    __builtin_amdgcn_wave_barrier();
                    const double *src = xpose + (lane >> 4) * XP_ROW + 4 * (lane & 15);
                    double t          = (src[0] + src[1]) + (src[2] + src[3]);
                    __builtin_amdgcn_wave_barrier();
                    t = dpp_step<0x111, 0xf>(t);
                    t = dpp_step<0x112, 0xf>(t);
                    t = dpp_step<0x114, 0xf>(t);
                    t = dpp_step<0x118, 0xf>(t);
                    if ((lane & 15) == 15 && t != 0.0) // (kb + 3 < Kp: every accumulator has Kp entries)
                        unsafeAtomicAdd(&lds_ev[s * Kp + kb + (lane >> 4)], t * H.scale); // RayTraceImageCPU.cpp:59, once per summed value
                }
            }
        }
    }
    // per seed: a negative intensity is error -2, a NaN in the I_ang sum error -3, after the sign test (Helper.h:582-594)
    unsigned failing = 0u, code = 0u;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            const bool bad_neg = iv_min[s] < 0.0, bad_nan = angsum[s] != angsum[s];
            if (bad_neg || bad_nan) {
                failing |= 1u << s;
                if (live && !safe_skip) {
                    const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
                    code |= c;
                    atomicOr(&H.ctl->seed_code[s], c);
                }
            }
        }
    }
    if (code) { // (live, not the skipping pass) one report per ray, whatever the number of seeds it fails under
        report_failure(code);
        if (safe_check)
            H.bad[ridx] = (unsigned char) failing; // the lane that holds the ray writes all its bits
    }
    if (safe_check)
        return;
    // runs of lanes with equal pixel, found once: the segmented scan of rt_step.hip; the last lane of a run owns the total
    const int pix_prev = __shfl_up(pix, 1, WAVE);
    const bool head    = lane == 0 || pix_prev != pix;
    int run_start      = head ? lane : -1;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int t = __shfl_up(run_start, o, WAVE);
        if (lane >= o && t > run_start)
            run_start = t;
    }
    const int head_next = __shfl_down(head ? 1 : 0, 1, WAVE);
    const bool tail     = (lane == WAVE - 1 || head_next != 0) && dep;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (s < n_seed) {
            // a ray that fails under seed s adds nothing to record s (RayTraceImageCPU.cpp:29-36: `continue` before the deposit)
            const bool ok = !((failing >> s) & 1u) && !((marked >> s) & 1u);
            if (ang >= 0 && ok) {
                if (lds_iang)
                    unsafeAtomicAdd(&lds_iang[s * seeds_ang_stride(H.n_ang) + ang], angsum[s]);
                else
                    unsafeAtomicAdd(&Q->out[s].iang[ang], angsum[s]);
            }
            double a = (dep && ok) ? angsum[s] * H.scale : 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double t = __shfl_up(a, 1 << i, WAVE);
                if ((lane - (1 << i)) >= run_start)
                    a += t;
            }
            if (tail && a != 0.0)
                unsafeAtomicAdd(&Q->out[s].nf[pix], a);
        }
    }
}

// One work-group of FREQ_WG_WAVES waves per CU, tiles handed out as rt_step_kernel hands them out.  LDS of a work-group,
// all dynamic (launch_step_seeds sizes it with step_seeds_lds_doubles):
//   [the two exponent tables][per seed: I_ang histogram, seeds_ang_stride(na*nb) doubles (if they fit)]
//   [per seed: E_v accumulator, Kp doubles][per wave: the transposition rows [4][XP_ROW] of the wave sum]
template <int SF>
__global__ void __launch_bounds__(FREQ_WG_WAVES * 64, FREQ_WAVES_SEED) rt_step_seeds_kernel(const SeedsKArg A)
{
    extern __shared__ __align__(16) unsigned char step_seeds_lds[];
    const FreqHot &H       = A.hot;
    const bool iang_in_lds = (H.flags & FQ_IANG_LDS) != 0;
    const int n_ang        = H.n_ang;
    const int n_seed       = A.set.n_seed;
    const int ang_stride   = seeds_ang_stride(n_ang);
    double *exp2_tab       = reinterpret_cast<double *>(step_seeds_lds);
    double *lds_iang       = iang_in_lds ? exp2_tab + 2 * EXP_TAB : nullptr;
    double *lds_ev         = exp2_tab + 2 * EXP_TAB + (iang_in_lds ? n_seed * ang_stride : 0);
    double *xpose          = lds_ev + n_seed * H.Kp + (size_t) (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)) * (size_t) (4 * XP_ROW);
    RT_FILL_EXP_TABLES(exp2_tab)
    if (lds_iang) {
        for (int c = (int) threadIdx.x; c < n_seed * ang_stride; c += (int) blockDim.x)
            lds_iang[c] = 0.0;
    }
    for (int c = (int) threadIdx.x; c < n_seed * H.Kp; c += (int) blockDim.x)
        lds_ev[c] = 0.0;
    __syncthreads();
    const int lane             = lane_id();
    const unsigned n_tiles_run = H.tile_end - H.tile_begin;
    unsigned shard = blockIdx.x & 7u, tried = 0;
    auto shard_size = [&](unsigned sh) { return (n_tiles_run + 7u - sh) / 8u; };
    unsigned s_n    = shard_size(shard);
    const unsigned sh_shift = H.fetch_shift > 3 ? H.fetch_shift - 3 : 0;
    auto chunk_of = [&](unsigned left) {
        const unsigned c = left >> sh_shift;
        return c < 1u ? 1u : (c > FREQ_TILES_PER_FETCH_GAIN ? FREQ_TILES_PER_FETCH_GAIN : c);
    };
    unsigned tch = chunk_of(s_n);
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
            // the cold half and the seed set of the argument block, the flag word and the lane number opaque per tile
            ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SeedsKArg, cold));
            SetPtr Q  = (SetPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SeedsKArg, set));
            asm volatile("" : "+s"(C), "+s"(Q));
            unsigned hflags = H.flags;
            int lane_t      = lane;
            asm volatile("" : "+s"(hflags), "+v"(lane_t));
            step_seeds_tile<SF>(H, hflags, C, Q, n_seed, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
        }
    }
    // the work-group's sums leave once, per seed: coalesced native f64 atomics (zeros stay)
    __syncthreads();
    for (int s = 0; s < n_seed; s++) {
        for (int c = (int) threadIdx.x; c < H.K; c += (int) blockDim.x) {
            const double v = lds_ev[s * H.Kp + c];
            if (v != 0.0)
                unsafeAtomicAdd(&A.set.out[s].E_v[c], v);
        }
        if (lds_iang && !(H.flags & FQ_DBG_NOFLUSH)) {
            for (int c = (int) threadIdx.x; c < n_ang; c += (int) blockDim.x) {
                const double v = lds_iang[s * ang_stride + c];
                if (v != 0.0)
                    unsafeAtomicAdd(&A.set.out[s].iang[c], v);
            }
        }
    }
}

} // namespace rt
