"""The whole per-step record -- the ASE triple and the triples of TWO seed beams -- at every plasma length n = 2 .. N two ways,
in one process, alternating within a step: device time of the march and of the second pass from the events, in step mode on
the ray grid, at N = 6 on the forward-emission stand-in (ASE_small x scale_problem(16), method 2; tables repeated and g0 scaled
per length as tests/length_scan.py does it), with the seeds `wide` and `narrow` of tests/ase_seeds.py.

  (a) a resident emission scan plan, and a resident scan plan of the same problem created with a seed (carry,
      tests/ase_seeds.py) that holds both seeds as its scan seeds, run back to back: two scan marches, two boundary buffers,
      rt_step_scan_kernel<true> and rt_step_scan_seeds_kernel -- what a caller had before
  (b) one emission scan plan with both seeds as its scan ASE seeds (rt_hip_plan_set_scan_ase_seeds): ONE march, one
      rt_step_scan_ase_seeds_kernel launch that leaves all 3 (N - 1) records

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  The predictions to test,
no threshold set in advance: (1) the march of (b) equals ONE scan march of (a) within the spread of the block medians; (2) the
pass of (b) lies between (a)'s emission scan pass and the sum of (a)'s two passes; (3) the total of (b) is below (a)'s by about
one scan march.

  python tools/scan_ase_seeds_ab.py [steps] [blocks] [out]          (this is how profiles/scan_ase_seeds_ab.txt was taken)"""
import importlib
import sys

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
import torch  # first: one HIP runtime in the process (tests/conftest.py, bench.py)

torch.zeros(1, device="cuda")
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
import ase_seeds as A
import length_scan as ls
import method_pairs as mp

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/scan_ase_seeds_ab.txt"
N = 6
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


p = mp.with_method(ls.scan_problem(mp.ase_forward(rt.scale_problem(rt.datfile.load('tests/golden/ASE_small.dat.xz'), 16.0)), N), 2)
seeds = [A.wide(p), A.narrow(p)]
q = A.carry(p, seeds[0])
scales = [q.scale, q.scale]
say(f"N = {N}; {steps} steps per block, {blocks} blocks, the ways alternating within a step; device times from the events, in ms")
pair = [be.Plan(p), be.Plan(q)]
one = be.Plan(p)
try:
    for plan in pair + [one]:
        plan.set_ray_grid().enable_step().enable_length_scan()
    pair[1].set_scan_seeds(seeds)
    one.set_scan_ase_seeds(seeds, scales)
    for _ in range(2):  # warm-up of both ways
        for plan in pair + [one]:
            plan.run()
            plan.kernel_times()
    med = {"a": [], "b": []}
    for _ in range(blocks):
        t = {"a": [], "b": []}
        for _ in range(steps):
            for plan in pair:
                plan.run()
            t["a"].append([x for plan in pair for x in plan.kernel_times()])
            one.run()
            t["b"].append(one.kernel_times())
        for w in t:
            med[w].append(np.median(np.array(t[w]), axis=0))
    full = one.fetch_full_length_steps()
    assert one.fetch(want_image=False)["failure_code"] == 0
    # (not a parity test -- tests/test_gpu_scan_ase_seeds.py gates the elements --: the two ways computed the same records)
    worst = 0.0
    for curve, ref_curve in zip([full["ase"]] + full["seeds"], [pair[0].fetch_length_steps()] + pair[1].fetch_seed_length_steps()):
        for rec, ref in zip(curve, ref_curve):
            for key in ("E_v", "nf", "I_ang"):
                d = np.linalg.norm(rec[key] - ref[key]) / np.linalg.norm(ref[key])
                worst = max(worst, d)
                assert d < 1e-12, (rec["n"], key, d)
finally:
    for plan in pair + [one]:
        plan.close()
a, b = np.array(med["a"]), np.array(med["b"])
a_march, a_pass = a[:, 0::2], a[:, 1::2]
say(f"\n== forward-emission stand-in (ASE_small x scale_problem(16), method 2): {p.n_rays_total} rays, nv {p.beam.nv}; two seeds, "
    f"{3 * (N - 1)} records (largest rel-L2 between a record of (b) and of (a): {worst:.2e})")
rows = [("(a) scan march of the emission plan", a_march[:, 0]), ("(a) scan march of the seeded plan", a_march[:, 1]),
        ("(a) rt_step_scan_kernel<true>", a_pass[:, 0]), ("(a) rt_step_scan_seeds_kernel", a_pass[:, 1]),
        ("(a) the two marches", a_march.sum(axis=1)), ("(a) the two passes", a_pass.sum(axis=1)), ("(a) kernel total", a.sum(axis=1)),
        ("(b) scan march", b[:, 0]), ("(b) rt_step_scan_ase_seeds_kernel", b[:, 1]), ("(b) kernel total", b.sum(axis=1))]
for what, v in rows:
    say(f"   {what:<42} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
one_march = np.median(a_march.mean(axis=1))
sp_march = max(spread(b[:, 0]), spread(a_march[:, 0]), spread(a_march[:, 1]))
d_march = np.median(b[:, 0]) / one_march - 1.0
say(f"   1. march of (b) against ONE scan march of (a) (the mean of its two): {100 * d_march:+.2f} % ({np.median(b[:, 0]) - one_march:+.3f} ms); spread "
    f"of the block medians {100 * sp_march:.2f} %: " + ("HOLDS, equal within the spread" if abs(d_march) <= sp_march else "DOES NOT HOLD, not equal within the spread"))
lo, hi, mine = np.median(a_pass[:, 0]), np.median(a_pass.sum(axis=1)), np.median(b[:, 1])
say(f"   2. pass of (b) {mine:.3f} ms against (a)'s emission scan pass {lo:.3f} ms (x {mine / lo:.3f}) and the sum of (a)'s two passes {hi:.3f} ms "
    f"(x {mine / hi:.3f}): " + ("HOLDS, between the two" if lo <= mine <= hi else "DOES NOT HOLD, not between the two"))
a_total, b_total = a.sum(axis=1), b.sum(axis=1)
sp_total = max(spread(a_total), spread(b_total))
saved = np.median(a_total) - np.median(b_total)
say(f"   3. kernel total of (b) against (a): {saved:+.3f} ms per step ({100 * saved / np.median(a_total):+.2f} %), ONE scan march of (a) is {one_march:.3f} ms, "
    f"the difference {saved - one_march:+.3f} ms ({100 * (saved - one_march) / np.median(a_total):+.2f} % of (a)'s total; spread of the block medians "
    f"{100 * sp_total:.2f} %): " + ("HOLDS, (b) is below (a) by one scan march within the spread" if abs(saved - one_march) <= sp_total * np.median(a_total)
                                   else "DOES NOT HOLD within the spread"))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
