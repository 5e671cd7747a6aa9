// rt_spec_scan_tile.inc -- what the tile functions of length spectra share: spec_scan_tile (rt_spec_scan.hip),
// spec_scan_seeds_tile (rt_spec_scan_seeds.hip), spec_scan_ase_seeds_tile (rt_spec_scan_ase_seeds.hip) and the two walks
// (rt_spec_scan_walk.inc, rt_spec_scan_seeds_walk.inc).
//
// Fragments of a function body (rt_tile_rec.inc says why text and not function templates); parameters are macros that the
// includer defines and undefines around the include.  The includer defines which part it wants.
//   SPEC_SCAN_HEAD      the tile head: the constants, the final state of the ray (rt_tile_ray.inc), the early return of a tile
//                       without rays, the segment the ray escaped in.  Reads BACKWARD, H, hflags, tile, lane.  Declares L, S, K,
//                       Kp, n_rays, row0, ridx, have, backward, rrec, rec, probe_on, what rt_tile_ray.inc declares, n_done,
//                       flags_steps, e_seg, skip.  (ridx and rrec are not const: spec_scan_ase_seeds_tile forms them anew
//                       between its halves.)
//   SPEC_SCAN_REC       the march record of this lane's ray (rt_tile_rec.inc; SF = 0: nothing to decode up front), and what of
//                       it a tile function of length spectra may leave unread.
//   SPEC_SCAN_STATE_AT  declares state_at(mseg): where the state lies that serves the blocks of m = mseg marched segments (the
//                       table of rt_spec_scan.hip) -- a boundary state or the final RecMeta, which begin with the same five
//                       floats (position, direction).  Reads Q->bnd, rec, rrec, ridx, L, S, e_seg, H.
//   SPEC_SCAN_STATE     the state that serves the blocks of m marched segments, once per tile and m: the -1 test of that state,
//                       the exit ray (stored here), the probe (that of the whole run: under m = L), the bit of error -1.
//                       Reads have, fl, steps, L, e_seg, ridx, blk_rays, probe_on, C, Q->out.ray2, e1m;
//                         SPEC_SCAN_STATE_SEG    m (1-based)
//                         SPEC_SCAN_STATE_HELD   (optional) the final state is the RecMeta `m` the head holds, a boundary state
//                                                is read over it (spec_scan_tile).  Without it the state is read where it
//                                                lies, so that no state is held across the seed factors (rt_step_rscan_seeds.hip)
//                         SPEC_SCAN_STATE_BY_LAMBDA  (optional, not HELD) ... through state_at, with which
//                                                spec_scan_ase_seeds_tile reads the state again in its seed half.  One form
//                                                for both did not hold: read in place rt_spec_scan_ase_seeds_kernel, through
//                                                the lambda rt_spec_scan_seeds_kernel came out with another stream.
//                         SPEC_SCAN_STATE_F0     (optional) statements: the includer's seed factors declared or zeroed, in
//                                                their place behind r2 (declared ahead of the state, the moves of
//                                                rt_spec_scan_kernel changed their order)
//                         SPEC_SCAN_STATE_BITS   statements of a state without error -1, behind its exit ray: the includer's
//                                                rule for its live and seed bits (they read bit, esc, skip, spx, spy, r2)
//                       Declares spx, spy, ssx, ssy, ssz, esc, bit, e1, r2 (not HELD: at_bnd).  The backward seed factors of
//                       a seed set at this state are the includer's, behind this part: SPEC_TILE_FACTORS of rt_spec_tile.inc.
//   SPEC_SCAN_FLUSH     the body of flush_row of the two walks: column `col` of the 64 staging rows to the row block at `blk`,
//                       frequencies kb .. kb + VEC - 1: 64 row pieces of 32 bytes, 16 bytes per lane and 32 rows per
//                       instruction; a last batch of two frequencies as one piece per row; ragged last tiles and odd K by
//                       8 bytes per lane.  Reads blk, col, kb, wide_ok, stage, lane, row0, n_rays, K.
//   SPEC_SCAN_CODES     the codes of a curve from its bits (error -1 of the state, a negative value seen, a NaN seen; one bit
//                       per length): per (curve, n) -1 of the state, else -2 over -3 (Helper.h:588-593: negative wins).
//                       Declares c, the code of the curve for this ray, which the includer reports once with the OR over its
//                       curves.  Statements, not a lambda: spec_scan_ase_seeds_tile wraps them in one (file_codes); called
//                       as a lambda rt_spec_scan_seeds_kernel came out with another stream.  Reads have, L, blk_rays, ridx,
//                       Q->out.err, e1m;
//                         SPEC_SCAN_CODES_CURVE   the curve: its row blocks are CURVE L .. CURVE L + L - 1
//                         SPEC_SCAN_CODES_NEG     its bits "a negative value seen", and
//                         SPEC_SCAN_CODES_NAN     "a NaN seen"
//                         SPEC_SCAN_CODES_WORD    (optional) the code word of the curve: takes c
#define SPEC_SCAN_STATE_PTR(mseg, at_bnd) \
    reinterpret_cast<const float *>(at_bnd ? Q->bnd + scan_bnd_off(ridx, mseg, L) : rec + rec_meta_off(rrec, S, H.rec_stride))
#if defined(SPEC_SCAN_HEAD)
    const int L           = H.L;
    const int S           = L * RT_N_SUB;
    const int K           = H.K;
    const int Kp          = H.Kp;
    const unsigned n_rays = H.n_rays;
    const unsigned row0   = tile * WAVE;
    unsigned ridx         = row0 + (unsigned) lane;
    const bool have       = ridx < n_rays;
    const bool backward   = BACKWARD;
    unsigned rrec            = have ? ridx : 0u;
    const unsigned char *rec = H.rec;
    const bool probe_on   = (hflags & FQ_PROBE) != 0;

    // ---- per-ray preamble, once: the final state of the ray (rt_tile_ray.inc) ----
#define TILE_NEED_RAY false
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
    (void) err1; // (of the final state: every block takes the test of its own state, SPEC_SCAN_STATE)
    if (__ballot(have) == 0ull)
        return;
    // the marched segment the ray escaped in (never: L + 1)
    const int n_done           = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
    const unsigned flags_steps = m.flags_steps;
    const int e_seg            = (fl & F_ESCAPED) ? (n_done > 0 ? (n_done - 1) / RT_N_SUB + 1 : 1) : L + 1;
    const bool skip            = (fl & F_SKIP) != 0u; // every update is the identity: rows of zeros at every n (with ASE seeds: in the ASE curve)
#elif defined(SPEC_SCAN_REC)
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
    (void) exact_emis;
#elif defined(SPEC_SCAN_STATE_AT)
    static_assert(offsetof(RecMeta, px) == 0 && offsetof(RecMeta, sz) == 16, "a boundary state and a RecMeta begin alike");
    auto state_at = [&](const int mseg) -> const float * {
        const bool at_bnd = mseg < L && mseg < e_seg;
        return SPEC_SCAN_STATE_PTR(mseg, at_bnd);
    };
#elif defined(SPEC_SCAN_STATE)
#ifdef SPEC_SCAN_STATE_HELD
    float spx = m.px, spy = m.py, ssx = m.sx, ssy = m.sy, ssz = m.sz;
    bool esc  = (fl & F_ESCAPED) != 0u;
    if (have && SPEC_SCAN_STATE_SEG < L && SPEC_SCAN_STATE_SEG < e_seg) {
        const float *q = reinterpret_cast<const float *>(Q->bnd + scan_bnd_off(ridx, SPEC_SCAN_STATE_SEG, L));
        spx            = q[0];
        spy            = q[1];
        ssx            = q[2];
        ssy            = q[3];
        ssz            = q[4];
        esc            = false;
    }
#else
    const bool at_bnd = SPEC_SCAN_STATE_SEG < L && SPEC_SCAN_STATE_SEG < e_seg;
    const bool esc    = !at_bnd && (fl & F_ESCAPED) != 0u;
    float spx = 0.0f, spy = 0.0f, ssx = 0.0f, ssy = 0.0f, ssz = 1.0f;
    if (have) {
#ifdef SPEC_SCAN_STATE_BY_LAMBDA
        const float *q = state_at(SPEC_SCAN_STATE_SEG);
#else
        const float *q = SPEC_SCAN_STATE_PTR(SPEC_SCAN_STATE_SEG, at_bnd);
#endif
        spx            = q[0];
        spy            = q[1];
        ssx            = q[2];
        ssy            = q[3];
        ssz            = q[4];
    }
#endif
    const unsigned bit = 1u << (SPEC_SCAN_STATE_SEG - 1);
    const bool e1      = have && (double) (ssz * ssz) < 0.01; // Helper.h:515
    rt_ray r2          = { 0.0f, 0.0f, 0.0f, 0.0f };          // (zeros under error -1, as rt_spec.hip leaves them)
#ifdef SPEC_SCAN_STATE_F0
    SPEC_SCAN_STATE_F0
#endif
    if (have && !e1) {
        r2.x = spx; // Helper.h:518-521
        r2.y = spy;
        r2.a = atanf_flt32_kernel(ssx / ssz) * 1e3f;
        r2.b = atanf_flt32_kernel(ssy / ssz) * 1e3f;
        SPEC_SCAN_STATE_BITS
    }
    if (e1)
        e1m |= bit;
    if (have) {
        Q->out.ray2[(size_t) (SPEC_SCAN_STATE_SEG - 1) * blk_rays + ridx] = r2;
        if (probe_on && SPEC_SCAN_STATE_SEG == L) { // the probe is that of the whole run
            C->probe.ray2[ridx]  = r2;
            C->probe.flags[ridx] = fl | (e1 ? F_ERR1 : 0u);
            C->probe.steps[ridx] = steps;
        }
    }
#elif defined(SPEC_SCAN_FLUSH)
    const int width = K - kb < VEC ? K - kb : VEC;
    if (wide_ok && width == VEC) {
        // two lanes cover the 32 staged bytes of a row, a store instruction 32 rows
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const unsigned row = (unsigned) (32 * g + (lane >> 1));
            SPEC_STORE16(stage + row * XS_ROW + col * VEC + 2 * (lane & 1), blk + ((size_t) (row0 + row) * (size_t) K + (size_t) (kb + 2 * (lane & 1))));
        }
    } else if (wide_ok) { // K = 4 i + 2: the last two frequencies of a row, one piece per lane
        SPEC_STORE16(stage + lane * XS_ROW + col * VEC, blk + ((size_t) (row0 + (unsigned) lane) * (size_t) K + (size_t) kb));
    } else {
        // ragged tile or odd K: 8 bytes per lane, sixteen rows per instruction
        const int k = kb + (lane & 3);
#pragma unroll
        for (int g = 0; g < WAVE / 16; g++) {
            const unsigned row = (unsigned) (16 * g + (lane >> 2));
            if (row0 + row < n_rays && k < K)
                blk[(size_t) (row0 + row) * (size_t) K + (size_t) k] = stage[row * XS_ROW + col * VEC + (lane & 3)];
        }
    }
#elif defined(SPEC_SCAN_CODES)
    if (have) {
#pragma unroll 1
        for (int jb = 0; jb < L; jb++) {
            const unsigned bit = 1u << jb;
            Q->out.err[((size_t) (SPEC_SCAN_CODES_CURVE) * (size_t) L + (size_t) jb) * blk_rays + ridx] =
                (e1m & bit) ? -1 : ((SPEC_SCAN_CODES_NEG & bit) ? -2 : ((SPEC_SCAN_CODES_NAN & bit) ? -3 : 0));
        }
    }
    const unsigned only_nan = SPEC_SCAN_CODES_NAN & ~SPEC_SCAN_CODES_NEG;
    const unsigned c        = (e1m ? 1u << 1 : 0u) | (SPEC_SCAN_CODES_NEG ? 1u << 2 : 0u) | (only_nan ? 1u << 3 : 0u);
#ifdef SPEC_SCAN_CODES_WORD
    if (c)
        atomicOr(&SPEC_SCAN_CODES_WORD, c);
#endif
#else
#error "rt_spec_scan_tile.inc: define SPEC_SCAN_HEAD, SPEC_SCAN_REC, SPEC_SCAN_STATE_AT, SPEC_SCAN_STATE, SPEC_SCAN_FLUSH or SPEC_SCAN_CODES"
#endif
#undef SPEC_SCAN_STATE_PTR
