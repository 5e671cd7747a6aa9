#pragma once
// rt_fused_step.hip -- step mode in ONE launch: the march and the step pass of a run as two phases of the same
// persistent waves, what rt_fused.hip does for image mode.  Opt-in (rt_hip_plan_set_step_one_launch, rt_launch.hip).
//
// Why: a step run is the run a time loop repeats, and as two kernels it ends twice -- the march's idle tail (rt_fused.hip
// says how long it is), then the ragged end of rt_step_kernel.  Nothing in the step pass needs a launch of its own:
// step_tile reads the tile-wise march records freq_tile reads, lanes = rays, and needs less LDS than the image pass --
// [4][XP_ROW] doubles per wave (no window totals, no row cache) and Kp doubles of E_v per work-group.
//
// Phase 1 is rt_fused_kernel's, statement for statement: set-up, table load, march_wave<true, BOUNDED, true, 1, OPT> with
// the TileList, the consumer waves, the late zone (host), buffer slots beside the tables and over them.  It is restated
// here and not shared as a function, so that every rt_fused_kernel instance keeps the instruction stream it was measured
// with.  Phase 2 pops tiles as rt_fused_kernel does and runs the step pass on each (step_tile_part below: step_tile's
// text, rt_tile_step.inc, and with it the deposit fragments rt_step_evsum.inc, rt_wave_runs.inc, rt_wave_runscan.inc), whole
// or on one of the four parts [k0, k1) of its frequency range (TILE_PART_FLAG); at the end the work-group flushes E_v and
// the I_ang histogram with f64 atomics, zeros skipped, as the epilogue of a step pass does (rt_step_wg.inc).
//
// Split tiles (the rules of freq_tile): a part integrates the batches k0 .. min(k1, K); error -1 is reported by the part
// with k0 == 0 only; E_v is per frequency anyway, and each part's share of the lane's sum over k goes into I_ang and nf
// by atomics -- a plain store into nf must not happen in a part, so the exclusive mode keeps two kernels (rt_launch.hip
// asserts it); a ray is tested for error -2 / -3 per part.  A failing run is repeated by the stand-alone rt_step_kernel
// (plan_repeat_checked), which starts the codes over.
//
// LDS: FusedLay's (rt_fused.hip) with per_wave = 4 XP_ROW, and Kp doubles of E_v behind the I_ang histogram, in front of
// off_ctl -- beside the tables, never under an overlaid buffer.  Their offset follows from off_iang and n_ang (FusedLay
// stays as it is: it is part of rt_fused_kernel's argument block).
#include "rt_fused.hip"
#include "rt_step.hip"

namespace rt {

struct FusedStepKArg {
    DevParams P;
    StepKArg S; // whole: step_tile finds nf through offsetof(StepKArg, out) - offsetof(StepKArg, cold) from the cold pointer
    unsigned *tile_next; // [4 n_tiles] links of the work-group tile lists
    FusedLay lay;
};
static_assert(sizeof(FusedStepKArg) <= 4096, "kernel argument segment");

// bytes from off_iang to the E_v accumulator (host: rt_launch.hip places off_ctl behind it)
__host__ __device__ inline unsigned fused_step_ev_off(int n_ang) { return (unsigned) ((n_ang + 1) & ~1) * (unsigned) sizeof(double); }

#pragma clang fp contract(fast) // (the float64 half, as in rt_step.hip)

// step_tile (rt_step.hip) on the frequencies [k0, k1) of a tile -- the same text, rt_tile_step.inc.  (A function of its
// own: with the range passed into step_tile, defaults 0 and 0x7fffffff, the four rt_step_kernel instances kept their
// registers but not their instruction streams.)
template <int SF, bool EMIS>
__device__ __forceinline__ void step_tile_part(const FreqHot &H, const unsigned hflags, ColdPtr C, double *lds_iang, double *lds_ev,
                                               const double *tab, double *xpose, const unsigned tile, const int lane, const int k0,
                                               const int k1)
{
#define TILE_K0 k0
#define TILE_K_END (k1 < K ? k1 : K)
#define TILE_REPORTS_ERR1 (k0 == 0)
#include "rt_tile_step.inc"
#undef TILE_K0
#undef TILE_K_END
#undef TILE_REPORTS_ERR1
}

template <bool BOUNDED, int SF, int OPT = 0>
__global__ void __launch_bounds__(1024) rt_fused_step_kernel(const FusedStepKArg A)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
#ifdef RT_WAVETIMES
    if (threadIdx.x == 0)
        atomicMin(&g_wt[2], __builtin_amdgcn_s_memrealtime()); // the first work-group to start: t = 0 of the launch
#endif
    const FreqHot &H   = A.S.hot;
    const int n_ang    = H.n_ang;
    double *exp2_tab   = reinterpret_cast<double *>(lds_raw + A.lay.off_exp);
    double *lds_iang   = reinterpret_cast<double *>(lds_raw + A.lay.off_iang);
    double *lds_ev     = reinterpret_cast<double *>(lds_raw + A.lay.off_iang + fused_step_ev_off(n_ang));
    unsigned *ctl      = reinterpret_cast<unsigned *>(lds_raw + A.lay.off_ctl);
    double *buf_free   = reinterpret_cast<double *>(lds_raw + A.lay.off_buf);
    const unsigned n_waves  = blockDim.x >> 6;
    const unsigned n_march  = n_waves - A.lay.n_consumers; // waves 0 .. n_march-1 march, the others only consume
    const unsigned wave_id  = (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const bool consumer     = A.lay.consumers_first ? wave_id < A.lay.n_consumers : wave_id >= n_march;
    // (everything below lies behind the march tables: the copy of the tables at the head of march_wave ends in the
    // barrier that also publishes these.  The transposition rows need no zeroing: step_tile writes all 64 columns of a
    // row before it reads them.)
    RT_FILL_EXP_TABLES(exp2_tab)
    for (int c = (int) threadIdx.x; c < n_ang; c += (int) blockDim.x)
        lds_iang[c] = 0.0;
    for (int c = (int) threadIdx.x; c < H.Kp; c += (int) blockDim.x)
        lds_ev[c] = 0.0;
    for (unsigned c = threadIdx.x; c < n_waves * 32u; c += blockDim.x)
        reinterpret_cast<unsigned *>(lds_raw + A.lay.off_rem)[c] = 0u;
    if (threadIdx.x == 0) {
        ctl[0] = TILE_NONE;
        ctl[1] = n_march;
        ctl[2] = 0u;
        ctl[3] = 0u;
    }
    const TileList list{ &ctl[0], A.tile_next, reinterpret_cast<unsigned *>(lds_raw + A.lay.off_nodes), &ctl[3], A.lay.node_cap,
                         reinterpret_cast<unsigned *>(lds_raw + A.lay.off_rem) + wave_id * 32u,
                         &ctl[1], n_march, A.lay.split, A.lay.k_part };

    // ---- phase 1: the march (rt_march.hip), one tile per chunk, finished tiles pushed onto the list ----
    march_load_tables<true>(A.P, lds_raw);
    if (!consumer)
        march_wave<true, BOUNDED, true, 1, OPT>(A.P, lds_raw, list);

    // ---- phase 2: this wave's rays have run out; step pass on the work-group's finished tiles ----
    const int lane = lane_id();
#ifdef RT_WAVETIMES // diagnostic build: {left the march, has a buffer, first tile done, end, where, tiles} per wave in g_ft
    const unsigned long long fu_left = __builtin_amdgcn_s_memrealtime();
    unsigned long long fu_first = 0, fu_tiles = 0;
#endif
    unsigned slot  = 0;
    if (lane == 0) {
        if (!consumer)
            __hip_atomic_fetch_add(&ctl[1], 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); // one marching wave less
        slot = __hip_atomic_fetch_add(&ctl[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    slot = (unsigned) __builtin_amdgcn_readfirstlane((int) slot);
    auto marching = [&]() { return __hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    double *xpose;
    if (slot < A.lay.n_free) {
        xpose = buf_free + (size_t) slot * A.lay.per_wave;
    } else {
        // a buffer over the march tables: not before the last wave of the work-group has stopped reading them
        while (marching() != 0u)
            __builtin_amdgcn_s_sleep(32);
        xpose = reinterpret_cast<double *>(lds_raw) + (size_t) (slot - A.lay.n_free) * A.lay.per_wave;
    }
#ifdef RT_WAVETIMES
    const unsigned long long fu_buf = __builtin_amdgcn_s_memrealtime();
#endif
    for (;;) {
        unsigned tile = TILE_NONE;
        if (lane == 0)
            tile = tile_pop(list);
        tile = (unsigned) __builtin_amdgcn_readfirstlane((int) tile);
        if (tile == TILE_NONE) {
            // nothing finished right now.  Tiles are pushed by marching waves only: once none is left the list can
            // only shrink, and an empty list then is the end (the pushes of a wave precede its leaving the march).
            if (marching() == 0u) {
                if (lane == 0)
                    tile = tile_pop(list);
                tile = (unsigned) __builtin_amdgcn_readfirstlane((int) tile);
                if (tile == TILE_NONE)
                    break;
            } else {
                __builtin_amdgcn_s_sleep(64);
                continue;
            }
        }
        // (as in rt_step_kernel: the cold half of the argument block is addressed inside the kernarg segment and made
        // opaque per tile, likewise the flag word and the lane number)
        ColdPtr C = (ColdPtr) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(FusedStepKArg, S) +
                               offsetof(StepKArg, cold));
        asm volatile("" : "+s"(C));
        unsigned hflags = H.flags;
        int lane_t      = lane;
        asm volatile("" : "+s"(hflags), "+v"(lane_t));
        // a whole tile, or one of the four parts of its frequency range (rt_march.hip: tile_publish)
        const unsigned part = (tile >> TILE_PART_SHIFT) & 3u;
        const int k0 = (tile & TILE_PART_FLAG) ? (int) (part * A.lay.k_part) : 0;
        const int k1 = (tile & TILE_PART_FLAG) && part < 3u ? k0 + (int) A.lay.k_part : 0x7fffffff;
        if (k0 < H.K)
            step_tile_part<SF, true>(H, hflags, C, lds_iang, lds_ev, exp2_tab, xpose, tile & TILE_ID_MASK, lane_t, k0, k1);
#ifdef RT_WAVETIMES
        if (!fu_first)
            fu_first = __builtin_amdgcn_s_memrealtime();
        fu_tiles++;
#endif
    }
#ifdef RT_WAVETIMES
    if (lane == 0) {
        const unsigned long long fu_end = __builtin_amdgcn_s_memrealtime();
        const unsigned w = atomicAdd(&g_ft_n, 1u);
        if (w < 8192) {
            g_ft[0][w] = fu_left;
            g_ft[1][w] = fu_buf;
            g_ft[2][w] = fu_first ? fu_first : fu_end;
            g_ft[3][w] = fu_end;
            g_ft[4][w] = (unsigned long long) blockIdx.x | ((unsigned long long) (threadIdx.x >> 6) << 16) | ((unsigned long long) slot << 24);
            g_ft[5][w] = fu_tiles;
        }
    }
#endif
    // the work-group's sums leave once.  (An epilogue of its own, not rt_step_wg.inc's: FusedLay always holds the histogram, and
    // it leaves unconditionally -- the shared text, with its two tests, is not this kernel's instruction stream.)
    __syncthreads();
    for (int c = (int) threadIdx.x; c < H.K; c += (int) blockDim.x) {
        const double v = lds_ev[c];
        if (v != 0.0)
            unsafeAtomicAdd(&A.S.out.E_v[c], v);
    }
    for (int c = (int) threadIdx.x; c < n_ang; c += (int) blockDim.x) {
        const double v = lds_iang[c];
        if (v != 0.0)
            unsafeAtomicAdd(&H.iang[c], v);
    }
}

} // namespace rt
