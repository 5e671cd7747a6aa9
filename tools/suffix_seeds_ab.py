"""The step records of two seed beams of the run of the last n lengths, n = 2 .. N, in the backward method, two ways, in one
process, alternating within a step: device time of the march and of the second pass from the events, in step mode on the ray
grid, at N = 6 (tables repeated and g0 scaled per length as tests/length_scan.py does it) on
method_pairs.seed_backward(seed_small) (seed_small.dat with method 1, 7.8 M rays on its seed-beam grid), with the seeds of
tests/suffix_seeds.py: the problem's own and the primed `narrow` profile.

  (a) two resident backward suffix-scan plans, run back to back, each created with one of the seeds -- two scan marches, two
      boundary buffers, rt_step_rscan_kernel<false> twice, both walking the same gl and taking the same exp: what a caller had
      before
  (b) one plan (created with seed 0) with both seeds installed (rt_hip_plan_set_suffix_seeds): ONE scan march, one
      rt_step_rscan_seeds_kernel launch that leaves all 2 (N - 1) records

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  A report, not a gate; no
threshold is fixed in advance.  Three comparisons are written down against the spread: the total of (b) against (a)'s, the
march of (b) against one march of (a) (the same instance on the same rays: equality is what one expects, and what was not
found in the two earlier measurements of this kind), and the pass of (b) as a multiple of one single-seed pass.

  python tools/suffix_seeds_ab.py [steps] [blocks] [out]     (this is how profiles/suffix_seeds_ab.txt was taken)"""
import importlib
import sys

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
import torch  # first: one HIP runtime in the process (tests/conftest.py, bench.py)

torch.zeros(1, device="cuda")
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
import length_scan as ls
import method_pairs as mp
import suffix_seeds as X

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/suffix_seeds_ab.txt"
N = 6
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


seed_small = rt.datfile.load('tests/golden/seed_small.dat.xz')
p = ls.scan_problem(mp.seed_backward(seed_small), N)
assert p.method == 1 and p.seed is not None and not p.use_emis
seeds = list(X.seeds_of(p, seed_small))
carried = [X.carry(p, s) for s in seeds]
say(f"N = {N}; {steps} steps per block, {blocks} blocks, the ways alternating within a step; device times from the events, in ms")
two = [be.Plan(q) for q in carried]
one = be.Plan(p)
try:
    for plan in two + [one]:
        plan.set_ray_grid().enable_step().enable_suffix_scan()
    one.set_suffix_seeds(seeds)
    for _ in range(2):  # warm-up of both ways
        for plan in two + [one]:
            plan.run()
            plan.kernel_times()
    med = {"a": [], "b": []}
    for _ in range(blocks):
        t = {"a": [], "b": []}
        for _ in range(steps):
            for plan in two:
                plan.run()
            t["a"].append([x for plan in two for x in plan.kernel_times()])
            one.run()
            t["b"].append(one.kernel_times())
        for w in t:
            med[w].append(np.median(np.array(t[w]), axis=0))
    curves = one.fetch_seed_length_steps()
    assert one.fetch(want_image=False)["failure_code"] == 0
    # (not a parity test -- tests/test_gpu_suffix_seeds.py gates the elements --: the two ways computed the same records)
    for curve, plan in zip(curves, two):
        for rec, ref in zip(curve, plan.fetch_length_steps()):
            for key in ("E_v", "nf", "I_ang"):
                d = np.linalg.norm(rec[key] - ref[key]) / np.linalg.norm(ref[key])
                assert d < 1e-11, (rec["n"], key, d)
finally:
    for plan in two + [one]:
        plan.close()
a, b = np.array(med["a"]), np.array(med["b"])
a_march, a_pass, a_total = a[:, 0::2].sum(axis=1), a[:, 1::2].sum(axis=1), a.sum(axis=1)
b_march, b_pass, b_total = b[:, 0], b[:, 1], b.sum(axis=1)
say(f"\n== seed_backward(seed_small), N = {N}: {p.n_rays_total} rays, nv {p.beam.nv}, seeds: its own and the primed `narrow` profile")
say("   kernels per step (zeroing launches apart): (a) 4, (b) 2")
names = ("the plan created with seed 0", "the plan created with seed 1")
rows = [(f"(a) scan march of {nm}", a[:, 2 * i]) for i, nm in enumerate(names)]
rows += [(f"(a) rt_step_rscan_kernel<false> of {nm}", a[:, 2 * i + 1]) for i, nm in enumerate(names)]
rows += [("(a) the two marches", a_march), ("(a) the two passes", a_pass), ("(a) kernel total", a_total),
         ("(b) scan march", b_march), ("(b) rt_step_rscan_seeds_kernel", b_pass), ("(b) kernel total", b_total)]
for what, v in rows:
    say(f"   {what:<62} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
sp_total = max(spread(a_total), spread(b_total))
gain = 1.0 - np.median(b_total) / np.median(a_total)
say(f"   1. kernel total of (b) against (a): {np.median(a_total) - np.median(b_total):+.3f} ms per step ({100 * gain:+.2f} % saved), spread of the block medians "
    f"{100 * sp_total:.2f} %: " + ("(b) is faster by more than the spread" if gain > sp_total else "(b) is NOT faster by more than the spread"))
m0 = np.median(a[:, 0])
sp_march = max(spread(b_march), spread(a[:, 0]))
d_march = np.median(b_march) / m0 - 1.0
say(f"   2. march: (b) {np.median(b_march):.3f} ms against the march of (a)'s plan created with seed 0 {m0:.3f} ms ({100 * d_march:+.2f} %; spread of the "
    f"block medians {100 * sp_march:.2f} %: " + ("within the spread" if abs(d_march) <= sp_march else "beyond the spread") +
    f"); (a)'s other march {np.median(a[:, 2]):.3f} ms; against the two marches {np.median(a_march):.3f} ms "
    f"({100 * (np.median(b_march) / np.median(a_march) - 1.0):+.2f} %)")
for i, nm in enumerate(names):
    one_pass = a[:, 2 * i + 1]
    say(f"   3. second pass: one rt_step_rscan_seeds_kernel {np.median(b_pass):.3f} ms is {np.median(b_pass) / np.median(one_pass):.3f} x the single-seed pass of "
        f"{nm} ({np.median(one_pass):.3f} ms; spread {100 * max(spread(b_pass), spread(one_pass)):.2f} %)")
say(f"      ... and against the two passes of (a) {np.median(a_pass):.3f} ms: {100 * (np.median(b_pass) / np.median(a_pass) - 1.0):+.2f} % "
    f"(spread {100 * max(spread(b_pass), spread(a_pass)):.2f} %)")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
