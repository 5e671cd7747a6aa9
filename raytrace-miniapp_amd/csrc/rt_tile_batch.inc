// rt_tile_batch.inc -- one frequency batch of one lane: Iv[0 .. VEC) of frequencies kb .. kb + VEC - 1 of the lane's ray,
// the emission recurrence over its sub-segments (Helper.h:549-557) or the gain-only product (Helper.h:569-580).
//
// A fragment of a function body, not a header: freq_tile (rt_freq.hip), spec_tile (rt_spec.hip) and step_tile
// (rt_step.hip) each include it inside their loop over kb, so the three modes run one definition of the arithmetic --
// every Iv_r[k] of spectra and step mode is the value image mode computes because it is the same text.
// (Text, not a function template: see rt_tile_rec.inc.)
//
// Reads from the including scope:
//   template parameters SF, EMIS; H, S, Kp, rec, rrec, m, backward, tab, f0, sfk, exact_emis, kb;
//   gs[], rs[], load_rows, all_regular, all_small, gv_nan            (rt_tile_rec.inc declares them)
//   TILE_READ_SLOT  the slot reader of the irregular and generic-S paths: rec_slot (rt_device.h, a select between two
//                   addresses: what the image kernels were built and measured with -- their SF = 0 instances keep 16 / 80
//                   bytes of scratch for its zero slot, and the other reader changes their code) or rec_slot_lazy
//                   (rt_freq.hip: the load behind the test, no scratch; spectra and step mode)
//   TILE_REREAD     the lane may read its record again on the irregular path (else e = 0): true in image mode, `have` in
//                   step mode, `live` in spectra mode, whose other lanes carry zeroed slots
//   TILE_BATCH_ROWS_LOADED   (optional, rt_step_ase_seeds.hip) the including scope has declared FVec w[SF] and loaded the
//                   rows of this batch itself, because something else reads them as well; undefined, the text is as it was
//   TILE_BATCH_SLOT(g, w)    (optional, likewise) statements on the gain sum and the row of every slot of the generic-S
//                   emission loop; undefined, nothing
// Writes: double Iv[VEC], declared by the including scope.  No masking: what a lane without a live ray gets is the
// including function's to drop; the padding columns K .. Kp-1 carry w = dv = 0, hence Iv = 0.
if (EMIS) {
#pragma unroll
    for (int j = 0; j < VEC; j++)
        Iv[j] = 0.0;
    if (SF) {
#ifndef TILE_BATCH_ROWS_LOADED
        FVec w[SF ? SF : 1];
        load_rows(w, kb);
#endif
        if (all_small) {
#pragma unroll
            for (int s = 0; s < SF; s++)
                ase_step_f32(Iv, gs[s], rs[s], w[s].v, tab + EXP_TAB);
        } else if (all_regular) {
#pragma unroll
            for (int s = 0; s < SF; s++)
                ase_step(Iv, gs[s], rs[s], w[s].v, tab);
        } else
#pragma unroll
        for (int s = 0; s < SF; s++) {
            if (fabsf(gs[s]) >= RT_RS_MIN && fabsf(gs[s]) <= H.gs_cap && !exact_emis) {
                ase_step(Iv, gs[s], rs[s], w[s].v, tab);
            } else {
                const float e1 = TILE_REREAD ? TILE_READ_SLOT(rec, rrec, H.rec_stride, s, SF, m.flags_steps, backward).e : 0.0f;
                if (gs[s] != 0.0f || e1 != 0.0f) { // else the update is the identity
#pragma unroll
                    for (int j = 0; j < VEC; j++)
                        Iv[j] = ase_update(Iv[j], gs[s], e1, w[s].v[j], tab);
                }
            }
        }
        if (gv_nan) {
#pragma unroll
            for (int j = 0; j < VEC; j++) {
                bool wn = false;
#pragma unroll
                for (int s = 0; s < SF; s++)
                    wn = wn || !(fabsf(w[s].v[j]) <= FLT_MAX);
                Iv[j] = wn ? __builtin_nan("") : Iv[j];
            }
        }
    } else {
        bool wnan[VEC]; // a NaN or infinity anywhere in this frequency's lineshape values (0 * NaN on the CPU)
#pragma unroll
        for (int j = 0; j < VEC; j++)
            wnan[j] = false;
        for (int s = 0; s < S; s++) {
            const RecSlot sl = TILE_READ_SLOT(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
            const float g1 = sl.g, e1 = sl.e;
            const int c1   = sl.c;
            const float *row  = H.gain[s / RT_N_SUB + 1].gv + (size_t) c1 * (size_t) Kp + kb;
            const FVec w = *reinterpret_cast<const FVec *>(row);
#pragma unroll
            for (int j = 0; j < VEC; j++)
                wnan[j] = wnan[j] || !(fabsf(w.v[j]) <= FLT_MAX);
#ifdef TILE_BATCH_SLOT
            TILE_BATCH_SLOT(g1, w)
#endif
            if (fabsf(g1) >= RT_RS_MIN && fabsf(g1) <= H.gs_cap && !exact_emis) {
                const double r1 = div_fast((double) e1, (double) g1);
                ase_step(Iv, g1, r1, w.v, tab);
            } else if (g1 != 0.0f || e1 != 0.0f) {
#pragma unroll
                for (int j = 0; j < VEC; j++)
                    Iv[j] = ase_update(Iv[j], g1, e1, w.v[j], tab);
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; j++)
            Iv[j] = wnan[j] ? __builtin_nan("") : Iv[j];
    }
} else {
    // gain only, Helper.h:569-580: f64 products summed in sub-segment order
    double gl[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++)
        gl[j] = 0.0;
    if (SF) {
        FVec w[SF ? SF : 1];
        load_rows(w, kb);
#pragma unroll
        for (int s = 0; s < SF; s++) {
#pragma unroll
            for (int j = 0; j < VEC; j++)
                gl[j] += (double) gs[s] * (double) w[s].v[j];
        }
    } else {
        for (int s = 0; s < S; s++) {
            const RecSlot sl = TILE_READ_SLOT(rec, rrec, H.rec_stride, s, S, m.flags_steps, backward);
            const float *row = H.gain[s / RT_N_SUB + 1].gv + (size_t) sl.c * (size_t) Kp + kb;
            const FVec w     = *reinterpret_cast<const FVec *>(row);
#pragma unroll
            for (int j = 0; j < VEC; j++)
                gl[j] += (double) sl.g * (double) w.v[j];
        }
    }
    // Iv = f0 f[4][k] exp(gl); for f0 = 0 that is exactly 0 unless exp overflows (0 * inf):
    // a wave none of whose lanes needs the exponential skips it
    bool need = f0 != 0.0;
#pragma unroll
    for (int j = 0; j < VEC; j++)
        need = need || gl[j] > 700.0 || gl[j] != gl[j];
#pragma unroll
    for (int j = 0; j < VEC; j++)
        Iv[j] = f0 * sfk[kb + j];
    if (__ballot(need) != 0ull) {
        double eg[VEC];
        exp_tab_vec(gl, tab, eg);
#pragma unroll
        for (int j = 0; j < VEC; j++)
            Iv[j] *= eg[j];
    }
}
