// rt_spec_wg.inc -- the work-group of a per-ray spectra pass: the size of its LDS on the host and the shell of its kernel, in
// one file so that neither changes without the other.  One work-group of FREQ_WG_WAVES waves per CU; LDS, all dynamic:
//   [the two exponent tables of rt_freq_kernel][per wave: [64][XS_ROW] staging doubles]
// Tiles are handed out from the eight sharded counters of the control block (DevCtl::next_tile_f, rt_freq_kernel says why
// eight), one tile per fetch: every tile costs the same here (the step passes reserve guided chunks, rt_step_handout.inc).
// Two parts; the includer defines which one it wants.
//   SPEC_WG_SIZE     namespace scope, once (rt_spec.hip): spec_lds_doubles
//   SPEC_WG_KERNEL   the whole body of a kernel whose argument block is `A`, hot half first, cold half behind it (rt_tile_rec.inc
//                    says why text and not a function template): rt_spec_kernel, rt_spec_scan_kernel, rt_spec_seeds_kernel,
//                    rt_spec_scan_seeds_kernel, rt_spec_ase_seeds_kernel and rt_spec_scan_ase_seeds_kernel.  Carves the LDS,
//                    fills the exponent tables, ends the prologue in a barrier and walks the tiles.  Per tile it forms the
//                    pointers to the blocks of the argument block behind the hot half, makes them, the flag word and the lane
//                    number opaque (as rt_freq_kernel, and as rt_step_scan_wg.inc does for the scan passes of step mode) and
//                    calls the tile function.  Reads
//                      SPEC_WG_KARG        the type of A (the offsetof of its blocks)
//                      SPEC_WG_BLOCK       (optional) the field of A behind the cold half (`scan`, `set`), and
//                      SPEC_WG_BLOCK_PTR   its pointer type: Q points to it
//                      SPEC_WG_CALL        the call of the tile function: reads H, hflags, C, [Q,] exp2_tab, stage, tile, lane_t
//                    Declares spec_lds[], H, exp2_tab, stage, lane, n_tiles_run, shard, tried, and in the loop t, tile, C, [Q,]
//                    hflags and lane_t.
// (What the tile function takes beside these -- the seed count of the four passes with seeds -- the kernel reads from its
// argument block before the include.  The six kernels are the ones their six copies of this shell gave, instruction for
// instruction: profiles/spectra_share_kernel_resources.txt, profiles/spectra_tiles_share_kernel_resources.txt.)
#if defined(SPEC_WG_SIZE)
// doubles of dynamic LDS of a work-group of wg_waves waves
inline size_t spec_lds_doubles(int wg_waves) { return (size_t) 2 * EXP_TAB + (size_t) wg_waves * WAVE * XS_ROW; }
#elif defined(SPEC_WG_KERNEL)
extern __shared__ __align__(16) unsigned char spec_lds[];
const FreqHot &H = A.hot;
double *exp2_tab = reinterpret_cast<double *>(spec_lds);
double *stage    = exp2_tab + 2 * EXP_TAB + (size_t) (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)) * (size_t) (WAVE * XS_ROW);
RT_FILL_EXP_TABLES(exp2_tab)
__syncthreads();
const int lane             = lane_id();
const unsigned n_tiles_run = H.tile_end - H.tile_begin;
unsigned shard = blockIdx.x & 7u, tried = 0;
#define SPEC_WG_PTR(T, field) (T) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SPEC_WG_KARG, field))
for (;;) {
    unsigned t = 0;
    if (lane == 0)
        t = atomicAdd(&H.ctl->next_tile_f[H.freq_id][shard][0], 1u);
    t = (unsigned) __builtin_amdgcn_readfirstlane((int) t);
    if (t >= (n_tiles_run + 7u - shard) / 8u) { // this shard is empty: on to the next one, until all eight have been seen empty
        if (++tried == 8)
            break;
        shard = (shard + 1) & 7u;
        continue;
    }
    const unsigned tile = H.tile_begin + t * 8u + shard;
    ColdPtr C = SPEC_WG_PTR(ColdPtr, cold);
#ifdef SPEC_WG_BLOCK
    SPEC_WG_BLOCK_PTR Q = SPEC_WG_PTR(SPEC_WG_BLOCK_PTR, SPEC_WG_BLOCK);
    asm volatile("" : "+s"(C), "+s"(Q));
#else
    asm volatile("" : "+s"(C));
#endif
    unsigned hflags = H.flags;
    int lane_t      = lane;
    asm volatile("" : "+s"(hflags), "+v"(lane_t));
    SPEC_WG_CALL
}
#undef SPEC_WG_PTR
#endif
