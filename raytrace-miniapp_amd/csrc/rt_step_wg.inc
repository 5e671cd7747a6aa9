// rt_step_wg.inc -- the LDS of a work-group of a step pass with n_rec records (the plain step pass: 1; a seed set: one per
// seed; a length scan: one per length): its size on the host, and the prologue and epilogue of the kernel around the tile
// hand-out (rt_step_handout.inc), in one file so that neither changes without the other.  All of it dynamic:
//   [the two exponent tables of rt_freq_kernel][n_rec I_ang histograms, ang_stride doubles apart (if they fit: FQ_IANG_LDS)]
//   [n_rec E_v accumulators, Kp doubles each][per wave: the transposition rows [4][XP_ROW] of the wave sum (rt_step_evsum.inc)]
// Three parts; the includer defines which one it wants.  The two kernel parts are fragments of a kernel body (rt_tile_rec.inc
// says why text) of rt_step_kernel, rt_step_seeds_kernel, rt_step_scan_kernel and rt_step_scan_seeds_kernel (one record per
// (seed, length)); rt_fused_step_kernel has FusedLay's layout.
//   STEP_WG_SIZE       namespace scope, once (rt_step.hip): step_ang_stride, seeds_ang_stride, step_lds_doubles
//   STEP_WG_PROLOGUE   carves the LDS, fills the exponent tables, zeroes histograms and accumulators, ends in a barrier.
//                      Reads H, A and
//                        STEP_WG_NREC         the number of records (an expression: 1, A.set.n_seed, H.L)
//                        STEP_WG_ANG_STRIDE   doubles from one histogram to the next (may name n_ang)
//                        STEP_WG_ANG_ZERO     doubles of the histograms to zero (the plain step pass: na * nb, not its stride)
//                      Declares step_lds[], iang_in_lds, n_ang, n_rec, ang_stride, exp2_tab, lds_iang, lds_ev, xpose.
//   STEP_WG_EPILOGUE   the work-group's sums leave once, record by record: coalesced native f64 atomics; zeros (most of a
//                      small launch's histogram) stay.  Reads what the prologue declared, H and
//                        STEP_WG_EV(r, c), STEP_WG_IANG(r, c)   entry c of E_v / cell c of I_ang of record r, lvalues
//                        STEP_WG_RECORD(r)    statements at the head of record r (what its two destinations share), or nothing
//                        STEP_WG_ONE_RECORD   defined where STEP_WG_NREC is the literal 1: the flush is a block with r = 0
// (The last two keep the kernels the ones the three copies gave, instruction for instruction,
// profiles/step_share_kernel_resources.txt: as a loop of one trip, which the compiler unrolls late, the flush changed the
// streams and SGPR spill counts of all four rt_step_kernel instances; with a record's base pointer formed inside the
// destinations, not once per record, the streams of both rt_step_scan_kernel instances.)
#if defined(STEP_WG_SIZE)
// doubles from one I_ang histogram in LDS to the next.  The plain step pass has one histogram: na * nb rounded up to even.
__host__ __device__ constexpr int step_ang_stride(int n_ang) { return (n_ang + 1) & ~1; }
// Several records: na * nb and two cells to spare (on an axis of one grid point the angle cell of a ray can be one past the
// grid, see rt_hip_plan_run; such a cell must not be the next record's), even
__host__ __device__ constexpr int seeds_ang_stride(int n_ang) { return (n_ang + 3) & ~1; }
// doubles of dynamic LDS of a work-group
// (ang_stride: step_ang_stride(n_ang) or seeds_ang_stride(n_ang), the one the kernel's prologue is given)
inline size_t step_lds_doubles(bool iang_in_lds, int ang_stride, int Kp, int wg_waves, int n_rec)
{
    return (size_t) 2 * EXP_TAB + (size_t) n_rec * ((iang_in_lds ? (size_t) ang_stride : 0) + (size_t) Kp) + (size_t) wg_waves * (size_t) (4 * XP_ROW);
}
#elif defined(STEP_WG_PROLOGUE)
extern __shared__ __align__(16) unsigned char step_lds[];
const bool iang_in_lds = (H.flags & FQ_IANG_LDS) != 0;
const int n_ang        = H.n_ang;
const int n_rec        = STEP_WG_NREC;
const int ang_stride   = STEP_WG_ANG_STRIDE;
double *exp2_tab       = reinterpret_cast<double *>(step_lds);
double *lds_iang       = iang_in_lds ? exp2_tab + 2 * EXP_TAB : nullptr;
double *lds_ev         = exp2_tab + 2 * EXP_TAB + (iang_in_lds ? n_rec * ang_stride : 0);
double *xpose          = lds_ev + n_rec * H.Kp + (size_t) (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)) * (size_t) (4 * XP_ROW);
RT_FILL_EXP_TABLES(exp2_tab)
if (lds_iang) {
    for (int c = (int) threadIdx.x; c < STEP_WG_ANG_ZERO; c += (int) blockDim.x)
        lds_iang[c] = 0.0;
}
for (int c = (int) threadIdx.x; c < n_rec * H.Kp; c += (int) blockDim.x)
    lds_ev[c] = 0.0;
__syncthreads();
#elif defined(STEP_WG_EPILOGUE)
__syncthreads();
#if defined(STEP_WG_ONE_RECORD)
{
    constexpr int r = 0;
#else
for (int r = 0; r < n_rec; r++) {
#endif
    STEP_WG_RECORD(r)
    for (int c = (int) threadIdx.x; c < H.K; c += (int) blockDim.x) {
        const double v = lds_ev[r * H.Kp + c];
        if (v != 0.0)
            unsafeAtomicAdd(&STEP_WG_EV(r, c), v);
    }
    if (lds_iang && !(H.flags & FQ_DBG_NOFLUSH)) {
        for (int c = (int) threadIdx.x; c < n_ang; c += (int) blockDim.x) {
            const double v = lds_iang[r * ang_stride + c];
            if (v != 0.0)
                unsafeAtomicAdd(&STEP_WG_IANG(r, c), v);
        }
    }
}
#else
#error "rt_step_wg.inc: define STEP_WG_SIZE, STEP_WG_PROLOGUE or STEP_WG_EPILOGUE"
#endif
