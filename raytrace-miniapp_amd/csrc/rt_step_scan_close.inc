// rt_step_scan_close.inc -- the close of one record of a chunk in the six scan passes of step mode, behind the chunk's walk:
// the failure test of Helper.h:582-594 on the lane's sum over k, and what the ray adds to the record's I_ang and nf.
// Error -2 (a negative Iv, NaNs ignored) or -3 (a NaN sum) under a record removes the ray from that record only
// (RayTraceImageCPU.cpp:29-36); the ray is reported once, by the includer, with the OR of its codes.
//
// Fragments of a function body (rt_tile_rec.inc says why text); the includer defines which part it wants.  Both read
//   SCAN_CLOSE_SUM      the lane's sum over k under this record (angsum[..])
//   SCAN_CLOSE_TEST     reads neg, safe_skip, code;
//                         SCAN_CLOSE_BIT      the bit of this record in `neg`
//                         SCAN_CLOSE_LIVE     the ray is live under this record
//                         SCAN_CLOSE_CODE     the code word of this record (len_code[jb], seed_len_code[s][jb], rec_len_code[r][jb])
//                         SCAN_CLOSE_MARK     statements: the mark of the checking repeat -- a bit of a word the includer
//                                             writes at the end of the tile, or the store itself where the marks are
//                                             written chunk by chunk (a chunk's records are its own)
//                         SCAN_CLOSE_FAILS    (optional) statements for a ray that fails under this record, live or not: where
//                                             the tests of all records of a length come first and the deposits behind the
//                                             runs of that length, the includer files a bit per record here.  The report
//                                             is then nested under the failure test and `failing` is not declared: with
//                                             one condition for both forms the forward kernels came out with other streams
//                       Declares bad_neg, bad_nan, failing; sets bit 2 or 3 in code and in the code word.
//   SCAN_CLOSE_DEPOSIT  where the checking pass of a failing run does not come.  Reads Q, H, lds_iang, lane, and run_start
//                       and tail of the runs of equal pixel the ray is in (rt_wave_runs.inc: forward per length, backward
//                       per tile);
//                         SCAN_CLOSE_OK       the ray adds to this record (live, not failing, not marked)
//                         SCAN_CLOSE_BLOCK    the record's block of Q->out and its histogram in LDS
//                         SCAN_CLOSE_ANG, SCAN_CLOSE_PIX   the ray's angle cell and pixel under this record (-1: none)
//                         SCAN_CLOSE_SCALE    the scale of the record's curve
//                         SCAN_CLOSE_RUNS     (optional) the runs are those of SCAN_CLOSE_PIX and are taken here, between the
//                                             two adds (one record per length: rt_step_scan.hip)
//                         SCAN_CLOSE_HAS_PIX  (optional) the bool the includer holds for SCAN_CLOSE_PIX >= 0 (backward: has_pix
//                                             of the tile; tested again here, rt_step_rscan_kernel<false> came out with
//                                             another stream); undefined, the test is taken here
//                       The I_ang add (LDS or global), the segmented nf scan (rt_wave_runscan.inc) and one atomic per run
//                       tail.  Declares nothing outside its block.
#if defined(SCAN_CLOSE_TEST)
const bool bad_neg = ((neg >> (SCAN_CLOSE_BIT)) & 1u) != 0u, bad_nan = SCAN_CLOSE_SUM != SCAN_CLOSE_SUM;
#ifdef SCAN_CLOSE_FAILS
if (bad_neg || bad_nan) {
    SCAN_CLOSE_FAILS
    if (SCAN_CLOSE_LIVE && !safe_skip)
#else
const bool failing = bad_neg || bad_nan;
if (SCAN_CLOSE_LIVE && failing && !safe_skip)
#endif
    {
        const unsigned c = bad_neg ? (1u << 2) : (1u << 3);
        code |= c;
        atomicOr(&SCAN_CLOSE_CODE, c);
        SCAN_CLOSE_MARK
    }
#ifdef SCAN_CLOSE_FAILS
}
#endif
#elif defined(SCAN_CLOSE_DEPOSIT)
{
    double *blk = Q->out + (size_t) (SCAN_CLOSE_BLOCK) * (size_t) Q->stride;
    if (SCAN_CLOSE_ANG >= 0 && SCAN_CLOSE_OK) {
        if (lds_iang)
            unsafeAtomicAdd(&lds_iang[(SCAN_CLOSE_BLOCK) * seeds_ang_stride(H.n_ang) + SCAN_CLOSE_ANG], SCAN_CLOSE_SUM);
        else
            unsafeAtomicAdd(&blk[Q->ang_off + (unsigned) SCAN_CLOSE_ANG], SCAN_CLOSE_SUM);
    }
#ifndef SCAN_CLOSE_HAS_PIX
    const bool has_px = SCAN_CLOSE_PIX >= 0;
#define SCAN_CLOSE_HAS_PIX has_px
#define SCAN_CLOSE_HAS_PIX_IS_DEFAULT
#endif
#ifdef SCAN_CLOSE_RUNS
#define RUNS_PIX SCAN_CLOSE_PIX
#define RUNS_DEPOSITS SCAN_CLOSE_HAS_PIX
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
#endif
    double a = (SCAN_CLOSE_HAS_PIX && SCAN_CLOSE_OK) ? SCAN_CLOSE_SUM * SCAN_CLOSE_SCALE : 0.0;
#include "rt_wave_runscan.inc"
    if (tail && a != 0.0)
        unsafeAtomicAdd(&blk[Q->nf_off + (unsigned) SCAN_CLOSE_PIX], a);
}
#ifdef SCAN_CLOSE_HAS_PIX_IS_DEFAULT
#undef SCAN_CLOSE_HAS_PIX
#undef SCAN_CLOSE_HAS_PIX_IS_DEFAULT
#endif
#else
#error "rt_step_scan_close.inc: define SCAN_CLOSE_TEST or SCAN_CLOSE_DEPOSIT"
#endif
