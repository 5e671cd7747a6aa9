// rt_wave_runscan.inc -- the sum of a value over each run of lanes found by rt_wave_runs.inc: six steps of an inclusive
// scan that does not cross the start of a run.  Behind it the last lane of a run (`tail`) holds the run's total; what
// becomes of the total -- a plain store, an atomic into an image row or into a record's nf -- is the includer's.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text); the includers of rt_wave_runs.inc, freq_tile
// once per frequency, step_seeds_tile once per seed.
//
// Reads from the including scope: lane, run_start;
//   a   a double the includer has declared and set to the lane's value (0.0 for a lane that adds nothing)
// Leaves in `a` the sum over the lanes of the run up to and including this one.
#pragma unroll
for (int i = 0; i < 6; i++) {
    const double t = __shfl_up(a, 1 << i, WAVE);
    if ((lane - (1 << i)) >= run_start)
        a += t;
}
