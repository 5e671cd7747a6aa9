// rt_wave_runs.inc -- the runs of consecutive lanes of a wave with equal pixel: the first half of the segmented scan of a
// deposit, rt_wave_runscan.inc the second.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text): the seeded deposit of freq_tile
// (rt_freq.hip) and rt_tile_step.inc include it once per tile, step_seeds_tile (rt_step_seeds.hip) once per tile for all
// seeds, step_scan_tile (rt_step_scan.hip) once per length; the unit test dm_nf_scan_kernel (rt_devmath.hip).
//
// Reads from the including scope: lane;
//   RUNS_PIX        the lane's pixel (-1: none; lanes without a pixel form runs of their own, which have no tail)
//   RUNS_DEPOSITS   this lane's ray deposits
// Declares: pix_prev, head (the lane starts a run), run_start (the first lane of the lane's run, by a max scan over the heads),
// head_next, tail (the last lane of a run of depositing lanes: it owns the run's total).
const int pix_prev = __shfl_up(RUNS_PIX, 1, WAVE);
const bool head    = lane == 0 || pix_prev != RUNS_PIX;
int run_start      = head ? lane : -1;
#pragma unroll
for (int o = 1; o < WAVE; o <<= 1) {
    const int t = __shfl_up(run_start, o, WAVE);
    if (lane >= o && t > run_start)
        run_start = t;
}
const int head_next = __shfl_down(head ? 1 : 0, 1, WAVE);
const bool tail     = (lane == WAVE - 1 || head_next != 0) && RUNS_DEPOSITS;
