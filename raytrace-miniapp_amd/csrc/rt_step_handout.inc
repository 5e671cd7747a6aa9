// rt_step_handout.inc -- the tile hand-out of a step pass: which tiles of the launch a wave takes, and the walk over them.
//
// A fragment of a kernel body, not a header (rt_tile_rec.inc says why text and not a function template): rt_step_kernel
// (rt_step.hip), rt_step_seeds_kernel (rt_step_seeds.hip), rt_step_scan_kernel (rt_step_scan.hip) and rt_step_scan_seeds_kernel
// (rt_step_scan_seeds.hip) include it once,
// between the work-group prologue and epilogue (rt_step_wg.inc).
//
// The eight sharded counters of the control block (DevCtl::next_tile_f, rt_freq_kernel says why eight): a wave starts on
// the shard of its work-group, reserves guided chunks -- (tiles left in the shard) >> shift, between 1 and
// HANDOUT_TILES_PER_FETCH -- and visits the other seven as a guest that takes single tiles.  rt_freq_kernel hands out by
// the same rule, as a single loop with a window of reserved tiles; rt_spec_kernel takes one tile per fetch.
//
// Reads from the including scope: H, lane;
//   HANDOUT_TILES_PER_FETCH   the cap of a reservation (FREQ_TILES_PER_FETCH_GAIN, or the choice by EMIS)
//   HANDOUT_TILE              the statements of one tile: they read `tile` and `lane`, make the blocks of the kernel's
//                             argument block behind the hot half, the flag word and the lane number opaque, and call the
//                             tile function
// Declares: n_tiles_run, shard, tried, shard_size, s_n, sh_shift, TILES_PER_FETCH, chunk_of, tch.
const unsigned n_tiles_run = H.tile_end - H.tile_begin;
unsigned shard = blockIdx.x & 7u, tried = 0;
auto shard_size = [&](unsigned sh) { return (n_tiles_run + 7u - sh) / 8u; };
unsigned s_n    = shard_size(shard);
const unsigned sh_shift = H.fetch_shift > 3 ? H.fetch_shift - 3 : 0;
constexpr unsigned TILES_PER_FETCH = HANDOUT_TILES_PER_FETCH;
auto chunk_of = [&](unsigned left) {
    const unsigned c = left >> sh_shift;
    return c < 1u ? 1u : (c > TILES_PER_FETCH ? TILES_PER_FETCH : c);
};
unsigned tch = chunk_of(s_n);
// (the reservation and the walk over its tiles as two nested loops: as rt_freq_kernel's single loop with a window of
// reserved tiles the gain-only instance kept 48 bytes of stack for its loop state)
for (;;) {
    unsigned base = 0;
    if (lane == 0)
        base = atomicAdd(&H.ctl->next_tile_f[H.freq_id][shard][0], tch);
    base = (unsigned) __builtin_amdgcn_readfirstlane((int) base);
    if (base >= s_n) { // this shard is empty: on to the next one, until all eight have been seen empty
        if (++tried == 8)
            break;
        shard = (shard + 1) & 7u;
        s_n   = shard_size(shard);
        tch   = 1; // a guest takes single tiles
        continue;
    }
    const unsigned t_end = s_n - base < tch ? s_n : base + tch;
    tch                  = chunk_of(s_n - t_end);
    for (unsigned t = base; t < t_end; t++) {
        const unsigned tile = H.tile_begin + t * 8u + shard;
        HANDOUT_TILE
    }
}
