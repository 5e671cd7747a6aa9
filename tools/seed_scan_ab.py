"""The gain-length curves of TWO seed beams -- the step record of either seed at every plasma length n = 2 .. N -- two ways,
in one process, alternating within a step: device time of the march and of the second pass from the events, in step mode on
the ray grid, at N = 6 on seed_small's full grid (tables repeated and g0 scaled per length as tests/length_scan.py does it:
the seeded shape of tools/length_scan_ab.py).  The seeds: the problem's own and `primed` of it (tests/seed_scan.py: f[4]
reversed, f0 x 0.37).

  (a) two resident single-seed scan plans, one created with each seed, run back to back: two marches, two boundary
      buffers, two rt_step_scan_kernel launches that compute the same exp(gl_j[k]) -- what a caller had before
  (b) one scan plan with both scan seeds (rt_hip_plan_set_scan_seeds): ONE march, one rt_step_scan_seeds_kernel launch that
      leaves all 2 (N - 1) records

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  The predictions to
test, no threshold set in advance: the march of (b) equals ONE march of (a) within the spread of the block medians; the pass
of (b) lies between one and two single-seed scan passes (the seed-set kernel measured 1.36 - 1.38 x a single-seed pass,
profiles/seed_set_ab.txt).

  python tools/seed_scan_ab.py [steps] [blocks] [out]          (this is how profiles/seed_scan_ab.txt was taken)"""
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
import seed_scan as ss

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/seed_scan_ab.txt"
N = 6
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
p0 = ls.scan_problem(seed, N)
p1 = ss.with_seed(p0, ss.primed(p0.seed), "primed seed")
say(f"N = {N}; {steps} steps per block, {blocks} blocks, the ways alternating within a step; device times from the events, in ms")
singles = [be.Plan(p0), be.Plan(p1)]
both = be.Plan(p0)
try:
    for plan in singles + [both]:
        plan.set_ray_grid().enable_step().enable_length_scan()
    both.set_scan_seeds([p0.seed, p1.seed])
    for _ in range(2):  # warm-up of both ways
        for plan in singles + [both]:
            plan.run()
            plan.kernel_times()
    med = {"a": [], "b": []}
    for _ in range(blocks):
        t = {"a": [], "b": []}
        for _ in range(steps):
            for plan in singles:
                plan.run()
            t["a"].append([x for plan in singles for x in plan.kernel_times()])
            both.run()
            t["b"].append(both.kernel_times())
        for w in t:
            med[w].append(np.median(np.array(t[w]), axis=0))
    curves = both.fetch_seed_length_steps()
    assert both.fetch(want_image=False)["failure_code"] == 0
    # (not a parity test -- tests/test_gpu_seed_scan.py gates the elements --: the two ways computed the same records)
    worst = 0.0
    for curve, plan in zip(curves, singles):
        for rec, ref in zip(curve, plan.fetch_length_steps()):
            for key in ("E_v", "nf", "I_ang"):
                d = np.linalg.norm(rec[key] - ref[key]) / np.linalg.norm(ref[key])
                worst = max(worst, d)
                assert d < 1e-12, (rec["n"], key, d)
finally:
    for plan in singles + [both]:
        plan.close()
a, b = np.array(med["a"]), np.array(med["b"])
a_march, a_pass = a[:, 0::2], a[:, 1::2]
say(f"\n== seed_small, seeded forward: {p0.n_rays_total} rays, nv {p0.beam.nv}; two seeds, {2 * (N - 1)} records "
    f"(largest rel-L2 between a record of (b) and of (a): {worst:.2e})")
rows = [(f"(a) scan march of the plan of seed {s}", a_march[:, s]) for s in range(2)]
rows += [(f"(a) rt_step_scan_kernel of seed {s}", a_pass[:, s]) for s in range(2)]
rows += [("(a) the two marches", a_march.sum(axis=1)), ("(a) the two rt_step_scan_kernel launches", a_pass.sum(axis=1)), ("(a) kernel total", a.sum(axis=1)),
         ("(b) scan march", b[:, 0]), ("(b) rt_step_scan_seeds_kernel", b[:, 1]), ("(b) kernel total", b.sum(axis=1))]
for what, v in rows:
    say(f"   {what:<42} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
one_march = np.median(a_march.mean(axis=1))
one_pass = np.median(a_pass.mean(axis=1))
sp_march = max(spread(b[:, 0]), spread(a_march[:, 0]), spread(a_march[:, 1]))
d_march = np.median(b[:, 0]) / one_march - 1.0
say(f"   march of (b) against ONE march of (a) (the mean of its two): {100 * d_march:+.2f} % ({np.median(b[:, 0]) - one_march:+.3f} ms); spread of the "
    f"block medians {100 * sp_march:.2f} %: " + ("equal within the spread" if abs(d_march) <= sp_march else "NOT equal within the spread"))
ratio = np.median(b[:, 1]) / one_pass
say(f"   pass of (b) against ONE single-seed scan pass of (a) (the mean of its two): x {ratio:.3f} "
    f"({'between one and two passes' if 1.0 <= ratio <= 2.0 else 'NOT between one and two passes'}); against both: "
    f"{np.median(b[:, 1]) - np.median(a_pass.sum(axis=1)):+.3f} ms")
a_total, b_total = a.sum(axis=1), b.sum(axis=1)
sp_total = max(spread(a_total), spread(b_total))
gain = 1.0 - np.median(b_total) / np.median(a_total)
say(f"   kernel total of (b) against (a): {np.median(a_total) - np.median(b_total):+.3f} ms per pair of curves ({100 * gain:+.2f} %), spread of the block "
    f"medians {100 * sp_total:.2f} %: " + ("(b) is faster by more than the spread" if gain > sp_total else "(b) is NOT faster by more than the spread"))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
