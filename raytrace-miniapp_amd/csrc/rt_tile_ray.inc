// rt_tile_ray.inc -- the per-ray preamble that the three frequency kernels share: the march record of the lane's ray and
// its launch ray, the err1 test of Helper.h:515, and the failure report.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why): freq_tile (rt_freq.hip), spec_tile
// (rt_spec.hip) and step_tile (rt_step.hip) include it once, at the top.
//
// The preamble of a tile is a chain of memory round trips, and with ~25 tiles per wave its latency is what the kernel
// is made of once the frequency loop is fast (measured: 0.50 of 1.00 ms with the loop compiled out): so every load
// that does not depend on another is issued up front -- meta, then the SF slots (records are tile-wise, rt_device.h:
// slot s of the 64 lanes is one contiguous run), then the launch ray.
//
// Reads from the including scope: template parameter SF; H, C, S, rec, rrec, ridx, have,
//   TILE_NEED_RAY   the tile needs the launch rays of its lanes (a failing ray whose tile did not loads its own when it
//                   is reported).  An expression, evaluated below where the three copies had it: declared ahead of this
//                   fragment, the same test gave the image kernels other instruction streams.
// Declares: fl, steps, ray, m, raw[], R, need_ray, err1, report_failure(code).
//
unsigned fl = 0, steps = 0;
rt_ray ray  = { 0, 0, 0, 0 };
RecMeta m   = { 0, 0, 0, 0, 1, 0 };
RecSlot raw[SF ? SF : 1]; // slots as stored; those the ray never entered are masked with n_done in rt_tile_rec.inc
#pragma unroll
for (int s = 0; s < (SF ? SF : 1); s++)
    raw[s] = RecSlot{ 0.0f, 0.0f, 0 };
const DevRays R = load_cold(&C->rays);
const bool need_ray = TILE_NEED_RAY;
if (have) {
    m = *reinterpret_cast<const RecMeta *>(rec + rec_meta_off(rrec, S, H.rec_stride));
    if (SF) {
        const unsigned char *slot0 = rec + rec_slot_off(rrec, 0, H.rec_stride);
#pragma unroll
        for (int s = 0; s < SF; s++)
            raw[s] = *reinterpret_cast<const RecSlot *>(slot0 + (size_t) s * REC_SLOT_ROW);
    }
    if (need_ray) {
        float ta, tb;
        load_ray(R, ridx, ray, ta, tb, false);
    }
    fl    = m.flags_steps & REC_FLAG_MASK;
    steps = m.flags_steps >> REC_STEPS_SHIFT;
}
// a failing ray: its code (1 << 1, 2, 3 for error -1, -2, -3) into the failure word, and its launch ray into the list
// of the first RT_N_FAILED_MAX failing rays
auto report_failure = [&](const unsigned code) {
    atomicOr(&H.ctl->failure_code, code);
    unsigned slot_f = atomicAdd(&H.ctl->n_failed, 1u);
    if (slot_f < RT_N_FAILED_MAX) {
        rt_ray r = ray;
        if (!need_ray) {
            float ta, tb;
            load_ray(R, ridx, r, ta, tb, false);
        }
        H.ctl->failed[slot_f] = r;
    }
};
const bool err1 = have && (double) (m.sz * m.sz) < 0.01; // Helper.h:515
