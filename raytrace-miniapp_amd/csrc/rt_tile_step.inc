// rt_tile_step.inc -- the body of the step pass of one tile: per-ray preamble, record decode, the frequency batches with
// the E_v wave sum, the failure test, and the deposit into I_ang and nf (rt_step.hip says what each is).
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text and not a function template): step_tile
// (rt_step.hip) includes it for a whole tile, step_tile_part (rt_fused_step.hip) for a tile or one of the four parts of its
// frequency range -- one definition of the step pass, and rt_step_kernel compiled from the text it always had.
//
// Reads from the including scope: template parameters SF, EMIS; H, hflags, C, lds_iang, lds_ev, tab, xpose, tile, lane,
//   TILE_K0, TILE_K_END   the frequencies [TILE_K0, TILE_K_END) this call integrates and deposits (multiples of VEC up to
//                         the end; expressions, may name K)
//   TILE_REPORTS_ERR1     this call reports error -1 of its rays (of the parts of a tile: the one with k0 == 0)
// A part adds its share of the lane's sum over k to I_ang and nf by atomics and tests its rays for error -2 / -3 on its own
// frequencies, as freq_tile does; the plain store into nf of the exclusive mode must not meet a part (rt_launch.hip).
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

// ---- per-ray preamble: exit ray, seed factor, deposit cells (image mode's: rt_tile_ray.inc, place_ray) ----
#define TILE_NEED_RAY (!(hflags & FQ_OWN_CELLS) || probe_on)
#include "rt_tile_ray.inc"
#undef TILE_NEED_RAY
double f0       = 0.0;
int pix = -1, ang = -1;
if (have && !err1) {
    const Placed P = place_ray(hflags, C, R, H.nx, backward, ridx, m, fl, ray);
    f0  = P.f0;
    pix = P.pix;
    ang = P.ang;
}
if (have && probe_on) {
    C->probe.flags[ridx] = fl | (err1 ? F_ERR1 : 0u);
    C->probe.steps[ridx] = steps;
}
if (err1 && !safe_skip && TILE_REPORTS_ERR1) // error -1: the ray is reported (once) and deposits nothing
    report_failure(1u << 1);
const bool live = have && !err1 && !(fl & F_SKIP) && !(safe_skip && H.bad[ridx]);
if (__ballot(live) == 0ull)
    return;
if (!live) {
    pix = -1;
    ang = -1;
}
// the pixel of this launch that only this ray deposits into (exclusive mode: the host has proved one ray per pixel)
int own_pix = -1;
if ((hflags & FQ_EXCLUSIVE) && have) {
    const unsigned j = ridx % (unsigned) H.ny, i = ridx / (unsigned) H.ny;
    own_pix          = (int) (i + j * (unsigned) H.nx);
}

// ---- the march record of this lane's ray, and the tile-wide choice of the update: image mode's, over every
// lane that holds a ray ----
#define TILE_MASK true
#include "rt_tile_rec.inc"
#undef TILE_MASK
const ConstF64 dv2 = (ConstF64) (unsigned long long) H.dv2;
const ConstF64 sfk = (ConstF64) (unsigned long long) H.seed_fk;

double angsum = 0.0; // RayTraceImageCPU.cpp:63-68, sequential in k like the CPU
double iv_min = 0.0; // min over k of Iv, NaNs ignored: negative <=> error -2 (Helper.h:582-594)
const bool dep = pix >= 0; // this lane's ray deposits into the image

for (int kb = TILE_K0; kb < TILE_K_END; kb += VEC) {
    double Iv[VEC];
#define TILE_READ_SLOT rec_slot_lazy
#define TILE_REREAD have
#include "rt_tile_batch.inc"
#undef TILE_READ_SLOT
#undef TILE_REREAD
    // (no masking of the lane's own sums, as in image mode: lanes without a live ray are dropped below; the padding
    // columns K .. Kp-1 carry w = dv = 0, hence Iv = 0)
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        iv_min = fmin(iv_min, Iv[j]);
        angsum += dv2[kb + j] * Iv[j]; // RayTraceImageCPU.cpp:66: (2.0 * dv) * Iv
    }
    if (!safe_check) { // the checking pass of a failing run integrates without depositing
        // E_v: the wave sum over the depositing lanes into the one accumulator
#define EV_SUM_DEPOSITS dep
#define EV_SUM_INDEX kb
#include "rt_step_evsum.inc"
#undef EV_SUM_DEPOSITS
#undef EV_SUM_INDEX
    }
}
// a NaN intensity makes the I_ang sum NaN (Helper.h:590-593: error -3, after the sign test)
const bool bad_neg = iv_min < 0.0, bad_nan = angsum != angsum;
const bool failing = bad_neg || bad_nan;
if (live && failing && !safe_skip) {
    report_failure(bad_neg ? (1u << 2) : (1u << 3));
    if (safe_check)
        H.bad[ridx] = 1;
}
if (safe_check)
    return;
// a failing ray adds nothing to I_ang (RayTraceImageCPU.cpp:29-36: `continue` before the deposit)
if (ang >= 0 && !failing) {
    if (lds_iang)
        unsafeAtomicAdd(&lds_iang[ang], angsum);
    else
        unsafeAtomicAdd(&H.iang[ang], angsum);
}
// nf: the same per-ray sum, scaled, summed over each run of lanes with equal pixel (the segmented scan of the
// seeded deposit, once per tile instead of once per frequency: rt_wave_runs.inc, rt_wave_runscan.inc); the last lane of a
// run owns the total
{
    const double mine  = (dep && !failing) ? angsum * H.scale : 0.0;
#define RUNS_PIX pix
#define RUNS_DEPOSITS dep
#include "rt_wave_runs.inc"
#undef RUNS_PIX
#undef RUNS_DEPOSITS
    double a = mine;
#include "rt_wave_runscan.inc"
    if (tail) {
        // (the output pointer is read from the argument block here, behind the cold half, rather than kept across the tile)
        double *nf_out = reinterpret_cast<const RT_CONST_AS StepOut *>(reinterpret_cast<const RT_CONST_AS char *>(C) + (offsetof(StepKArg, out) - offsetof(StepKArg, cold)))->nf;
        if (pix == own_pix)
            nf_out[pix] = a; // the only ray of this pixel in the launch: a run of one lane, nothing to add to
        else if (a != 0.0)
            unsafeAtomicAdd(&nf_out[pix], a);
    }
}
