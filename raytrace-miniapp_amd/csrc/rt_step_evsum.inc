// rt_step_evsum.inc -- E_v of a step pass: the sum of a frequency batch over the depositing lanes of a wave, added to the
// work-group's accumulator in LDS.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text): rt_tile_step.inc, step_seeds_tile
// (rt_step_seeds.hip, once per seed) and step_scan_tile (rt_step_scan.hip, once per length) include it behind the
// integration of a batch, where the checking pass of a failing run does not come; the unit test dm_ev_sum_kernel
// (rt_devmath.hip) includes it alone.
//
// The wave sum of the few-runs deposit (wave_sums, rt_freq.hip, which leaves its totals in a window instead): the lanes park
// their VEC values in [4][XP_ROW], lane (j, q) = (lane / 16, lane % 16) adds four neighbours of frequency j, a row_shr tree
// finishes the sum in lane 15 of the row; one LDS atomic per frequency and tile, a zero sum adds nothing.
//
// Reads from the including scope: Iv[VEC], xpose, lane, lds_ev, H.scale, kb (through EV_SUM_INDEX);
//   EV_SUM_DEPOSITS   this lane's ray deposits (into this record)
//   EV_SUM_INDEX      index in lds_ev of the accumulator entry of frequency kb.  It is substituted without parentheses,
//                     `lds_ev[EV_SUM_INDEX + (lane >> 4)]`: as `(lds_ev + index)[lane >> 4]` nine instruction streams
//                     changed.  (kb + 3 < Kp: every accumulator has Kp entries.)
//   EV_SUM_SCALE      (optional) the scale of this record where it is not H.scale (rt_step_ase_seeds.hip: one scale per
//                     record); undefined, H.scale as ever
// Declares nothing outside its block.
#ifndef EV_SUM_SCALE
#define EV_SUM_SCALE H.scale
#define EV_SUM_SCALE_IS_DEFAULT
#endif
{
#pragma unroll
    for (int j = 0; j < VEC; j++)
        xpose[j * XP_ROW + lane] = EV_SUM_DEPOSITS ? Iv[j] : 0.0;
    __builtin_amdgcn_wave_barrier();
    const double *src = xpose + (lane >> 4) * XP_ROW + 4 * (lane & 15);
    double t          = (src[0] + src[1]) + (src[2] + src[3]);
    __builtin_amdgcn_wave_barrier();
    t = dpp_step<0x111, 0xf>(t);
    t = dpp_step<0x112, 0xf>(t);
    t = dpp_step<0x114, 0xf>(t);
    t = dpp_step<0x118, 0xf>(t);
    if ((lane & 15) == 15 && t != 0.0)
        unsafeAtomicAdd(&lds_ev[EV_SUM_INDEX + (lane >> 4)], t * EV_SUM_SCALE); // RayTraceImageCPU.cpp:59, once per summed value
}
#ifdef EV_SUM_SCALE_IS_DEFAULT
#undef EV_SUM_SCALE
#undef EV_SUM_SCALE_IS_DEFAULT
#endif
