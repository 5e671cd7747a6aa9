"""A/B of the march against the parent commit's library in one process: the stand-in, ASE_small, the rank-0 shard of an
8-rank run and seed_small, the two libraries alternating in both orders, best of 10 kernel times (march + frequency) each.

  python tools/step_prune_ab.py [out.txt [new.so]]   (csrc/librt_hip_prev.so = the parent's build, csrc/librt_hip.so or
                                                      csrc/new.so = this one)
"""
import importlib, sys
sys.path.insert(0, '.')
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
mg = importlib.import_module("raytrace-miniapp_amd.multigpu")
libs = {"prev": be.HipLibrary(be.CSRC / "librt_hip_prev.so"), "new": be.HipLibrary(be.CSRC / (sys.argv[2] if len(sys.argv) > 2 else "librt_hip.so"))}
base = rt.datfile.load('tests/golden/ASE_small.dat.xz')
standin = rt.scale_problem(base, 16.0)
cases = {"standin": standin, "ASE_small": base, "shard8": mg.shard(standin, 0, 8),
         "seed_small": rt.datfile.load('tests/golden/seed_small.dat.xz')}
lines = ["case        order      prev ms   new ms   new/prev - 1"]
for name, p in cases.items():
    plans = {}
    for k, lib in libs.items():
        plans[k] = be.Plan(p, lib=lib)
        plans[k].set_ray_grid()
        for _ in range(3):   # warm-up
            plans[k].run()
            plans[k].fetch(want_image=False)
    res = {}
    for order in (("prev", "new"), ("new", "prev")):
        best = {"prev": 1e9, "new": 1e9}
        for rnd in range(10):
            for k in order:
                plans[k].run()
                st = plans[k].fetch(want_image=False)["stats"]
                best[k] = min(best[k], st["march_ms"] + st["freq_ms"])
        res[order] = best
        lines.append(f"{name:11s} {order[0]}-first {best['prev']:8.4f} {best['new']:8.4f}   {100.0 * (best['new'] / best['prev'] - 1):+.2f} %")
    a, b = res[("prev", "new")], res[("new", "prev")]
    spread = max(abs(a["prev"] - b["prev"]), abs(a["new"] - b["new"]))
    gain = min(a["prev"] - a["new"], b["prev"] - b["new"])
    lines.append(f"{name:11s} order-to-order spread {spread:.4f} ms, smaller gain {gain:+.4f} ms = {gain / spread if spread > 0 else float('inf'):.1f} spreads")
    for plan in plans.values():
        plan.close()
    print("\n".join(lines[-3:]), flush=True)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
