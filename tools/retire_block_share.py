"""Diagnostic: what the retirement of finished rays costs a marching wave, and how often it runs (rt_march.hip, "ray
finished").  The timed build (make -C raytrace-miniapp_amd/csrc librt_hip_time.so): wave clock between the marks that
enclose the retirement block, and -- where the build has them -- the wave-iteration counters of g_retire.  For the
stand-in, seed_small, ASE_small and the rank-0 shard of an 8-rank run.

  python tools/retire_block_share.py [lib.so [label]] >> profiles/retire_block_share.txt
"""
import ctypes as C, importlib, sys
sys.path.insert(0, '.')
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
mg = importlib.import_module("raytrace-miniapp_amd.multigpu")
name = sys.argv[1] if len(sys.argv) > 1 else "librt_hip_time.so"
lib = be.HipLibrary(be.CSRC / name)
have = hasattr(lib.lib, "rt_hip_debug_retire_counters")
base = rt.datfile.load('tests/golden/ASE_small.dat.xz')
standin = rt.scale_problem(base, 16.0)
cases = {"standin": standin, "seed_small": rt.datfile.load('tests/golden/seed_small.dat.xz'), "ASE_small": base,
         "shard8": mg.shard(standin, 0, 8)}
print(f"== {sys.argv[2] if len(sys.argv) > 2 else name}" + ("" if have else "  (no g_retire counters in this build: clock shares only)"))
print("case         rays  wave-iters  DONE share  DONE clk/iter | iters with a ray finishing  retire block runs  rays/run  refills  iters/refill  iters dry")
for case, p in cases.items():
    with be.Plan(p, lib=lib) as plan:
        plan.set_ray_grid().run()
        out, ret = (C.c_ulonglong * 8)(), (C.c_ulonglong * 4)()
        lib.lib.rt_hip_debug_counters(out)      # discard the warm-up
        if have:
            lib.lib.rt_hip_debug_retire_counters(ret)
        plan.run()
        st = plan.fetch(want_image=False)["stats"]
        lib.lib.rt_hip_debug_counters(out)
        if have:
            lib.lib.rt_hip_debug_retire_counters(ret)
    v, r = list(out), list(ret)
    tot, it = sum(v[:6]), max(v[7], 1)
    line = f"{case:10s} {st['n_rays']:8d} {it:10d}  {100.0 * v[3] / tot:8.2f} %  {v[3] / it:12.1f}  |"
    if have:
        # (iterations per refill: of the iterations before the wave's ray counters ran dry -- there is no refill after)
        line += (f" {100.0 * r[0] / it:22.1f} %  {100.0 * r[1] / it:14.1f} %  {st['n_rays'] / max(r[1], 1):8.2f} {r[2]:8d}"
                 f"  {(it - r[3]) / max(r[2], 1):12.2f}  {100.0 * r[3] / it:7.1f} %")
    print(line, flush=True)
