// rt_step_scan_state.inc -- the state that serves a length (forward scan) or a record (suffix scan) of the six scan passes of
// step mode, and error -1 under it.  L = N - 1 marched segments; m segments into its march the ray crossed boundary m, whose
// state the scan instance of the march stored tile-wise (rt_march.hip MARCH_OPT_SCAN, scan_bnd_off: indexed by the number of
// segments marched, whatever the method); e = e_seg, the segment the ray escaped in (never: L + 1).  The table:
//   not escaped, m < L      boundary m                          not escaped, m = L      the final RecMeta
//   escaped,     m < e      boundary m, the ray NOT escaped     escaped,     m >= e     the final RecMeta, escaped
// (a ray found outside by the first test of segment m + 1 has e = m + 1: under m it has not escaped).  Error -1 under m is
// s.z^2 < 0.01 of that state (Helper.h:515): it sets bit 1 of the ray's code and of the code words of every record of m,
// and keeps the ray out of them.
//
// Fragments of a function body (rt_tile_rec.inc says why text).  All read have, fl, L, e_seg, ridx, Q, safe_skip, code and
//   SCAN_STATE_SEG         m (1-based)
//   SCAN_STATE_REPORT(b)   statements: atomicOr of bit 1 into the code words of block b = m - 1 of every record
//   SCAN_STATE_SILENT      (optional) no report and no code bit: another half of the tile function reports this m
// and declare e1.  The includer defines which form it wants:
//   SCAN_STATE_FORWARD   the state as a RecMeta and a flag word, and the placement of the ray under it: what the forward
//                        method deposits at.  Reads m, hflags, C, R, H, backward, ray;
//                          SCAN_STATE_PLACED   the statements of a ray that is placed under m: they read P, flj
//                        (the probe's exit ray is that of the whole run: written under m = L only).
//                        Declares mj, flj.
//   SCAN_STATE_HELD      backward, from a copy `mc` of the final RecMeta that the includer reads per chunk (five registers
//                        that need not live across the frequency loops).  Declares spx, spy, ssx, ssy, ssz, esc; what the
//                        includer does not read of them costs nothing.
//   SCAN_STATE_READ      backward, read where it lies: a boundary state and a RecMeta begin with the same five floats
//                        (position, direction), so that no state is held across the seed factors.  Reads rec, rrec, S, H.
//                        Declares at_bnd, esc, spx, spy, ssx, ssy, ssz.
//   SCAN_STATE_FACTORS   behind SCAN_STATE_READ: the seed factors of a seed set at that state's position and exit angles
//                        (place_ray's backward half, Helper.h:518-529; rscan_seed_factor), 0 where the ray has escaped by m.
//                        One copy of the text per accumulator: the seeds in a loop the compiler does not unroll, the factor
//                        filed by selects (inlined per (seed, accumulator) the kernels kept a stack frame).  Reads lv (the
//                        ray is live under some seed), Z->tabs, n_seed, NS, i; sets f0[.][i].
#define SCAN_STATE_BND reinterpret_cast<const float *>(Q->bnd + scan_bnd_off(ridx, SCAN_STATE_SEG, L))
#if defined(SCAN_STATE_FACTORS)
if (lv && !esc) {
    const float ea = atanf_flt32_kernel(ssx / ssz) * 1e3f;
    const float eb = atanf_flt32_kernel(ssy / ssz) * 1e3f;
#pragma unroll 1
    for (int s = 0; s < n_seed; s++) {
        const double f = rscan_seed_factor(&Z->tabs.seed[s], (double) spx, (double) spy, (double) ea, (double) eb);
#pragma unroll
        for (int t = 0; t < NS; t++)
            f0[t][i] = t == s ? f : f0[t][i];
    }
}
#else
#if defined(SCAN_STATE_FORWARD)
RecMeta mj   = m;
unsigned flj = fl;
if (have && SCAN_STATE_SEG < L && SCAN_STATE_SEG < e_seg) {
    const float *q = SCAN_STATE_BND;
    mj.px          = q[0];
    mj.py          = q[1];
    mj.sx          = q[2];
    mj.sy          = q[3];
    mj.sz          = q[4];
    flj            = fl & ~(unsigned) F_ESCAPED;
}
const float ssz = mj.sz;
#elif defined(SCAN_STATE_HELD)
float spx = mc.px, spy = mc.py, ssx = mc.sx, ssy = mc.sy, ssz = mc.sz;
bool esc  = (fl & F_ESCAPED) != 0u;
if (have && SCAN_STATE_SEG < L && SCAN_STATE_SEG < e_seg) {
    const float *q = SCAN_STATE_BND;
    spx            = q[0];
    spy            = q[1];
    ssx            = q[2];
    ssy            = q[3];
    ssz            = q[4];
    esc            = false;
}
(void) spx;
(void) spy;
(void) ssx;
(void) ssy;
(void) esc;
#elif defined(SCAN_STATE_READ)
static_assert(offsetof(RecMeta, px) == 0 && offsetof(RecMeta, sz) == 16, "a boundary state and a RecMeta begin alike");
const bool at_bnd = SCAN_STATE_SEG < L && SCAN_STATE_SEG < e_seg;
const bool esc    = !at_bnd && (fl & F_ESCAPED) != 0u;
float spx = 0.0f, spy = 0.0f, ssx = 0.0f, ssy = 0.0f, ssz = 1.0f;
if (have) {
    const float *q = at_bnd ? SCAN_STATE_BND : reinterpret_cast<const float *>(rec + rec_meta_off(rrec, S, H.rec_stride));
    spx            = q[0];
    spy            = q[1];
    ssx            = q[2];
    ssy            = q[3];
    ssz            = q[4];
}
#else
#error "rt_step_scan_state.inc: define SCAN_STATE_FORWARD, SCAN_STATE_HELD, SCAN_STATE_READ or SCAN_STATE_FACTORS"
#endif
const bool e1 = have && (double) (ssz * ssz) < 0.01; // Helper.h:515
#ifndef SCAN_STATE_SILENT
if (e1 && !safe_skip) { // reported once per ray, by the includer, with the OR of its codes
    code |= 1u << 1;
    SCAN_STATE_REPORT(SCAN_STATE_SEG - 1)
}
#endif
#if defined(SCAN_STATE_FORWARD)
if (have && !e1) {
    const unsigned pf = (hflags & ~(unsigned) (FQ_HAS_SEED | FQ_PROBE)) | (SCAN_STATE_SEG == L ? (hflags & (unsigned) FQ_PROBE) : 0u);
    const Placed P    = place_ray(pf, C, R, H.nx, backward, ridx, mj, flj, ray);
    SCAN_STATE_PLACED
}
#endif
#endif
#undef SCAN_STATE_BND
