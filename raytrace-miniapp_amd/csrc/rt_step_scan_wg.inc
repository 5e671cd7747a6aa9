// rt_step_scan_wg.inc -- the kernel shell of the six scan passes of step mode: rt_step_scan_kernel, rt_step_scan_seeds_kernel,
// rt_step_scan_ase_seeds_kernel and the three rt_step_rscan*_kernel.  The whole body of a kernel whose argument block is `A`
// -- hot half, cold half, ScanArg `scan`, and behind them the seed set `set` of the four passes that carry one: the shell of
// every step pass (rt_step_wg.inc, rt_step_handout.inc) with one record per block of A.scan.out, `stride` doubles apart, per
// record an I_ang histogram, seeds_ang_stride(na*nb) doubles apart, and an E_v accumulator.
//
// A fragment of a kernel body (rt_tile_rec.inc says why text and not a function template), in the manner of SPEC_WG_KERNEL
// (rt_spec_wg.inc).  Reads from the including scope: A;
//   SCAN_WG_KARG              the type of A (the offsetof of its blocks)
//   SCAN_WG_NREC              the number of records (H.L, A.set.n_seed * H.L, (1 + A.set.n_seed) * H.L)
//   SCAN_WG_TILES_PER_FETCH   the cap of a reservation (rt_step_handout.inc)
//   SCAN_WG_TILE              the tile function: (H, hflags, C, Q, [Z, n_seed,] lds_iang, lds_ev, exp2_tab, xpose, tile, lane)
//   SCAN_WG_SET               (optional) the pointer type of the seed set: Z points to A.set and A.set.n_seed is handed on
// Per tile the pointers to the blocks behind the hot half, the flag word, the lane number and the seed count are made opaque.
// Declares H, lane, and what rt_step_wg.inc and rt_step_handout.inc declare.
// (rt_step_seeds_kernel and rt_step_ase_seeds_kernel keep their own shells: their records are SeedOut blocks, not A.scan.)
const FreqHot &H = A.hot;
#define STEP_WG_NREC SCAN_WG_NREC
#define STEP_WG_ANG_STRIDE seeds_ang_stride(n_ang)
#define STEP_WG_ANG_ZERO n_rec * ang_stride
#define STEP_WG_RECORD(r) double *blk = A.scan.out + (size_t) r * (size_t) A.scan.stride;
#define STEP_WG_EV(r, c) blk[c]
#define STEP_WG_IANG(r, c) blk[A.scan.ang_off + c]
#define STEP_WG_PROLOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_PROLOGUE
const int lane = lane_id();
#define HANDOUT_TILES_PER_FETCH SCAN_WG_TILES_PER_FETCH
#define SCAN_WG_BLOCK(T, field) (T) ((const RT_CONST_AS char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SCAN_WG_KARG, field))
#ifdef SCAN_WG_SET
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C     = SCAN_WG_BLOCK(ColdPtr, cold);                                                                                      \
    ScanPtr Q     = SCAN_WG_BLOCK(ScanPtr, scan);                                                                                      \
    SCAN_WG_SET Z = SCAN_WG_BLOCK(SCAN_WG_SET, set);                                                                                   \
    asm volatile("" : "+s"(C), "+s"(Q), "+s"(Z));                                                                                      \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    int n_seed_t    = A.set.n_seed;                                                                                                    \
    asm volatile("" : "+s"(hflags), "+v"(lane_t), "+s"(n_seed_t));                                                                     \
    SCAN_WG_TILE(H, hflags, C, Q, Z, n_seed_t, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
#else
#define HANDOUT_TILE                                                                                                                   \
    ColdPtr C = SCAN_WG_BLOCK(ColdPtr, cold);                                                                                          \
    ScanPtr Q = SCAN_WG_BLOCK(ScanPtr, scan);                                                                                          \
    asm volatile("" : "+s"(C), "+s"(Q));                                                                                               \
    unsigned hflags = H.flags;                                                                                                         \
    int lane_t      = lane;                                                                                                            \
    asm volatile("" : "+s"(hflags), "+v"(lane_t));                                                                                     \
    SCAN_WG_TILE(H, hflags, C, Q, lds_iang, lds_ev, exp2_tab, xpose, tile, lane_t);
#endif
#include "rt_step_handout.inc"
#undef HANDOUT_TILES_PER_FETCH
#undef HANDOUT_TILE
#undef SCAN_WG_BLOCK
#define STEP_WG_EPILOGUE
#include "rt_step_wg.inc"
#undef STEP_WG_EPILOGUE
#undef STEP_WG_NREC
#undef STEP_WG_ANG_STRIDE
#undef STEP_WG_ANG_ZERO
#undef STEP_WG_RECORD
#undef STEP_WG_EV
#undef STEP_WG_IANG
