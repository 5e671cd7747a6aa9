// rt_tile_rec.inc -- the sub-segments of a lane's ray as the frequency update takes them, the tile-wide choice of the
// update, and the loader of a batch's lineshape rows.
//
// A fragment of a function body, not a header: freq_tile (rt_freq.hip), spec_tile (rt_spec.hip) and step_tile
// (rt_step.hip) include it once, after their per-ray preamble (rt_tile_ray.inc) and before their loop over the
// frequency batches (rt_tile_batch.inc).
// (Text, not function templates.  The same statements behind __device__ __forceinline__ templates came out of the
// compiler with other register counts: extracting this decode loop alone, verbatim, with references to the same arrays,
// took rt_freq_kernel<6, false, false> from 94 to 99 VGPRs and from five to four waves per SIMD; all the pieces
// together, as structs by value, changed 27 of the 64 kernel instances; profiles/tile_share_kernel_resources.txt.
// Included as text the kernels are the ones the three copies gave.  RT_FILL_EXP_TABLES, rt_freq.hip, is a macro for the
// same reason.)
//
// Reads from the including scope: template parameter SF; H, hflags, Kp, m, raw[], backward;
//   TILE_MASK   false zeroes the slots of the lane.  Spectra mode passes `live` -- the rows of its other lanes must be
//               zeros, and they must not steer the tile-wide choice --; image and step mode pass true: there the choice
//               is taken over every lane that holds a ray, live or not (the choice decides the arithmetic, and step
//               mode's arithmetic is image mode's), and what a lane without a live ray integrates is dropped later.
// Declares: gs[], rs[], off[], exact_emis, irregular, idle, all_regular, big, all_small, gv_nan, load_rows.
//
// off[s]: byte offset of the lineshape row of sub-segment s inside its length's table (32 bits:
// rt_hip_plan_create refuses tables of 4 GiB), so that a row load is SGPR base + VGPR offset
float gs[SF ? SF : 1];
double rs[SF ? SF : 1]; // es/gs, the source function of the sub-segment (see ase_step)
unsigned off[SF ? SF : 1];
const bool exact_emis = (hflags & FQ_EXACT_EMIS) != 0;
bool irregular = false;
if (SF) {
    const int n_done = (int) ((m.flags_steps >> REC_NDONE_SHIFT) & REC_NDONE_MASK);
#pragma unroll
    for (int s = 0; s < SF; s++) {
        // (rec_slot's rule on the slots loaded up front: only the first n_done in marching order were written)
        const bool written = TILE_MASK && (backward ? s >= SF - n_done : s < n_done);
        const RecSlot sl   = written ? raw[s] : RecSlot{ 0.0f, 0.0f, 0 };
        gs[s]              = sl.g;
        const float e1   = sl.e;
        off[s]           = (unsigned) sl.c * (unsigned) Kp * 4u;
        // regular: the source-function form (ase_step) takes this sub-segment; not when the gain
        // sum is tiny or NaN, and never in the exact mode (rt_hip_plan_set_exact_emission), which
        // runs the CPU's own formula with its per-frequency division throughout
        // (|gs| <= gs_cap keeps |gs * gv| <= 708 for every lineshape value; NaN fails both tests)
        const bool regular = fabsf(gs[s]) >= RT_RS_MIN && fabsf(gs[s]) <= H.gs_cap && !exact_emis;
        rs[s]              = regular ? div_fast((double) e1, (double) gs[s]) : 0.0;
        // (a sub-segment with both sums zero is the identity either way: x = 0, e^x - 1 = 0)
        irregular = irregular || (!regular && (gs[s] != 0.0f || e1 != 0.0f));
    }
}
// every |gs w| of the lane stays below 80 (the rule): the float32 range reduction (ase_step_f32)
bool big  = false;
bool idle = false; // a slot with gs = 0: the identity (with es != 0 the lane is irregular already)
if (SF) {
#pragma unroll
    for (int s = 0; s < SF; s++) {
        big  = big || !(fabsf(gs[s]) <= H.gs_cap * (80.0f / 708.0f));
        idle = idle || gs[s] == 0.0f;
    }
}
// no irregular sub-segment in the whole tile (the rule): the six updates of a frequency batch run
// as one straight-line block, so the table reads of one overlap the arithmetic of another.
// That block runs an identity slot as an update with e^x - 1 = 0: exact while Iv is finite, 0 * inf = NaN once Iv has
// overflowed, where the CPU keeps the infinity (Helper.h:549-557: Iv (1 + gl (1 + gl / 2)) with gl = 0) and the ray does
// not fail.  Iv cannot overflow while every |gs w| <= 80: |Iv| <= SF max |rs| e^(80 SF) with |rs| <= FLT_MAX / RT_RS_MIN,
// 6e277 for SF = 6.  So a lane that is big AND holds an identity slot (an escaped ray: the slots it never wrote) sends
// its tile to the per-slot branch, which skips identities.
const bool all_regular = __ballot(irregular || (idle && big)) == 0ull;
const bool all_small   = all_regular && __ballot(big) == 0ull;
// a NaN or an infinity among the lineshape values (the CPU's 0 * NaN, 0 * inf and inf / inf: every one of them
// leaves Iv = NaN, Helper.h:549-557) is tested per frequency only when the host scan of the tables found one
const bool gv_nan = (hflags & FQ_GV_NAN) != 0;

// row of sub-segment s, frequencies kb .. kb+3 (SF: the tables of lengths 1 and 2 are kernel arguments)
auto load_rows = [&](FVec (&w)[SF ? SF : 1], const int kb) {
#pragma unroll
    for (int s = 0; s < (SF ? SF : 1); s++) {
        const float *base = (s < RT_N_SUB ? H.gv0 : H.gv1) + kb;
        // (opaque here, so that the zero-extension of the offset stays beside the load and the
        // instruction selector finds the SGPR-base + 32-bit-VGPR-offset form)
        unsigned o = off[s];
        asm volatile("" : "+v"(o));
#ifdef RT_ABL_NOLOAD // profiling only
        o &= 15u;
#endif
        w[s] = *reinterpret_cast<const FVec *>(reinterpret_cast<const char *>(base) + o);
    }
};

