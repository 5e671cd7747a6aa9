"""The whole step record -- the ASE triple and the triple of two seed beams -- of the run of the last n lengths, n = 2 .. N, in
the backward method, two ways, in one process, alternating within a step: device time of the march and of the second pass
from the events, in step mode on the ray grid, at N = 6 (tables repeated and g0 scaled per length as tests/length_scan.py does
it) on the backward-emission stand-in (ASE_small x scale_problem(16), method 1, 6.4 M rays on its own grid), with the seeds
`wide` and `narrow` of tests/ase_seeds.py.

  (a) three resident suffix-scan plans, run back to back: the emission plan and two backward plans of the same problem created
      with one seed each (ase_seeds.carry) -- three scan marches, three boundary buffers, rt_step_rscan_kernel<true> once and
      rt_step_rscan_kernel<false> twice: what a caller had before
  (b) the emission plan with both seeds installed (rt_hip_plan_set_suffix_ase_seeds): ONE scan march, one
      rt_step_rscan_ase_seeds_kernel launch that leaves all 3 (N - 1) records

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  A report, not a gate; no
threshold is fixed in advance.  The expectation: the march of (b) is one of the three marches of (a), within the spread, and
the kernel total drops by more than the spread; the pass of (b) walks, per ray and frequency batch, the 18 sub-segments of the
emission half and 21 of the seed half where the three passes of (a) walk 18 + 21 + 21.

  python tools/suffix_ase_seeds_ab.py [steps] [blocks] [out]     (this is how profiles/suffix_ase_seeds_ab.txt was taken)"""
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

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/suffix_ase_seeds_ab.txt"
N = 6
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
p = ls.scan_problem(rt.scale_problem(ase, 16.0), N)
assert p.method == 1 and p.seed is None and p.use_emis
seeds = list(A.seeds_of(p))
carried = [A.carry(p, s) for s in seeds]
scales = [q.scale for q in carried]
say(f"N = {N}; {steps} steps per block, {blocks} blocks, the ways alternating within a step; device times from the events, in ms")
three = [be.Plan(p)] + [be.Plan(q) for q in carried]
one = be.Plan(p)
try:
    for plan in three + [one]:
        plan.set_ray_grid().enable_step().enable_suffix_scan()
    one.set_suffix_ase_seeds(seeds, scales)
    for _ in range(2):  # warm-up of both ways
        for plan in three + [one]:
            plan.run()
            plan.kernel_times()
    med = {"a": [], "b": []}
    for _ in range(blocks):
        t = {"a": [], "b": []}
        for _ in range(steps):
            for plan in three:
                plan.run()
            t["a"].append([x for plan in three for x in plan.kernel_times()])
            one.run()
            t["b"].append(one.kernel_times())
        for w in t:
            med[w].append(np.median(np.array(t[w]), axis=0))
    full = one.fetch_full_length_steps()
    assert one.fetch(want_image=False)["failure_code"] == 0
    # (not a parity test -- tests/test_gpu_suffix_ase_seeds.py gates the elements --: the two ways computed the same records)
    for curve, plan in zip([full["ase"]] + full["seeds"], three):
        for rec, ref in zip(curve, plan.fetch_length_steps()):
            for key in ("E_v", "nf", "I_ang"):
                d = np.linalg.norm(rec[key] - ref[key]) / np.linalg.norm(ref[key])
                assert d < 1e-5, (rec["n"], key, d)
finally:
    for plan in three + [one]:
        plan.close()
a, b = np.array(med["a"]), np.array(med["b"])
a_march, a_pass, a_total = a[:, 0::2].sum(axis=1), a[:, 1::2].sum(axis=1), a.sum(axis=1)
b_march, b_pass, b_total = b[:, 0], b[:, 1], b.sum(axis=1)
say(f"\n== backward-emission stand-in (ASE_small x scale_problem(16), method 1): {p.n_rays_total} rays, nv {p.beam.nv}, seeds `wide` and `narrow`")
say("   kernels per step (zeroing launches apart): (a) 6, (b) 2")
names = ("the emission plan", "the plan created with `wide`", "the plan created with `narrow`")
rows = [(f"(a) scan march of {nm}", a[:, 2 * i]) for i, nm in enumerate(names)]
rows += [(f"(a) rt_step_rscan_kernel of {nm}", a[:, 2 * i + 1]) for i, nm in enumerate(names)]
rows += [("(a) the three marches", a_march), ("(a) the three passes", a_pass), ("(a) kernel total", a_total),
         ("(b) scan march", b_march), ("(b) rt_step_rscan_ase_seeds_kernel", b_pass), ("(b) kernel total", b_total)]
for what, v in rows:
    say(f"   {what:<58} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
m0 = np.median(a[:, 0])
say(f"   march: (b) {np.median(b_march):.3f} ms against the emission plan's march of (a) {m0:.3f} ms ({100 * (np.median(b_march) / m0 - 1.0):+.2f} %; spread of the "
    f"block medians {100 * max(spread(b_march), spread(a[:, 0])):.2f} %) and against the three marches {np.median(a_march):.3f} ms "
    f"({100 * (np.median(b_march) / np.median(a_march) - 1.0):+.2f} %)")
say(f"   second pass: one rt_step_rscan_ase_seeds_kernel {np.median(b_pass):.3f} ms against the three passes of (a) {np.median(a_pass):.3f} ms "
    f"({100 * (np.median(b_pass) / np.median(a_pass) - 1.0):+.2f} %; spread {100 * max(spread(b_pass), spread(a_pass)):.2f} %)")
sp_total = max(spread(a_total), spread(b_total))
gain = 1.0 - np.median(b_total) / np.median(a_total)
say(f"   kernel total of (b) against (a): {np.median(a_total) - np.median(b_total):+.3f} ms per step ({100 * gain:+.2f} % saved), spread of the block medians "
    f"{100 * sp_total:.2f} %: " + ("(b) is faster by more than the spread" if gain > sp_total else "(b) is NOT faster by more than the spread"))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
