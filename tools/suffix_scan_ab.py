"""The gain-length curve in the backward method -- the step record of the run of the last n lengths, n = 2 .. N -- two ways,
in one process, alternating blocks: device time of the march and of the second pass from the events, in step mode on the
ray grid, at N = 6 (tables repeated and g0 scaled per length as tests/length_scan.py does it) on the backward-emission
stand-in (ASE_small x scale_problem(16), method 1, 6.4 M rays on its own grid) and on seed_backward(seed_small).

  (a) N - 1 resident step plans of the suffix problems (problem.suffix_lengths), run back to back: 1 + 2 + ... + (N - 1)
      plasma segments marched, N - 1 step kernels -- what a caller had before
  (b) one plan with the suffix scan on: ONE backward march of N - 1 segments that also stores the boundary states, one
      rt_step_rscan_kernel launch that leaves all N - 1 records
  (c) a plain step plan of all N lengths, for the march of (b) to be compared with: the difference is the price of the
      boundary stores (and of the pruning the scan instance goes without).  The plain march instances are, instruction for
      instruction, those of the commit before the suffix scan (profiles/suffix_scan_kernel_resources.txt).

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  A report, not a gate.
The arithmetic predicts that (b) marches 5 segments where (a) marches 15, two thirds of the march time saved at N = 6, and
that the pass of (b) walks 18 (emission: chunks of four suffixes) or 21 (gain-only: three) sub-segments per ray and
frequency batch where the five passes of (a) walk 45.

  python tools/suffix_scan_ab.py [steps] [blocks] [out]          (this is how profiles/suffix_scan_ab.txt was taken)"""
import importlib
import sys

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
import torch  # first: one HIP runtime in the process (tests/conftest.py, bench.py)

torch.zeros(1, device="cuda")
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
import length_scan as ls
import method_pairs as mp

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/suffix_scan_ab.txt"
N = 6
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
say(f"N = {N}; {steps} steps per block, {blocks} blocks per shape, the ways alternating within a step; device times from the events, in ms")
shapes = (("backward-emission stand-in (ASE_small x scale_problem(16), method 1)", ls.scan_problem(rt.scale_problem(ase, 16.0), N)),
          ("seed_small, seeded backward", ls.scan_problem(mp.seed_backward(seed), N)))
for name, p in shapes:
    suffix_plans = [be.Plan(problem_mod.suffix_lengths(p, n)) for n in range(2, N + 1)]
    scan, plain = be.Plan(p), be.Plan(p)
    try:
        for plan in suffix_plans + [scan, plain]:
            plan.set_ray_grid().enable_step()
        scan.enable_suffix_scan()
        for _ in range(2):  # warm-up of every way
            for plan in suffix_plans + [scan, plain]:
                plan.run()
                plan.kernel_times()
        med = {"a": [], "b": [], "c": []}
        for _ in range(blocks):
            t = {"a": [], "b": [], "c": []}
            for _ in range(steps):
                for plan in suffix_plans:
                    plan.run()
                t["a"].append([x for plan in suffix_plans for x in plan.kernel_times()])
                scan.run()
                t["b"].append(scan.kernel_times())
                plain.run()
                t["c"].append(plain.kernel_times())
            for w in t:
                med[w].append(np.median(np.array(t[w]), axis=0))
        recs = scan.fetch_length_steps()
        assert scan.fetch(want_image=False)["failure_code"] == 0
        # (not a parity test -- tests/test_gpu_suffix_scan.py gates the elements --: the two ways computed the same records)
        for rec, plan in zip(recs, suffix_plans):
            ref = plan.fetch_step()
            for key in ("E_v", "nf", "I_ang"):
                d = np.linalg.norm(rec[key] - ref[key]) / np.linalg.norm(ref[key])
                assert d < 1e-5, (name, rec["n"], key, d)
    finally:
        for plan in suffix_plans + [scan, plain]:
            plan.close()
    a, b, c = np.array(med["a"]), np.array(med["b"]), np.array(med["c"])
    a_march, a_step, a_total = a[:, 0::2].sum(axis=1), a[:, 1::2].sum(axis=1), a.sum(axis=1)
    b_march, b_scan, b_total = b[:, 0], b[:, 1], b.sum(axis=1)
    say(f"\n== {name}: {p.n_rays_total} rays, nv {p.beam.nv}")
    say(f"   kernels per curve (zeroing launches apart): (a) {2 * (N - 1)}, (b) 2")
    rows = [(f"(a) march of the plan of the last n = {n}", a[:, 2 * i]) for i, n in enumerate(range(2, N + 1))]
    rows += [("(a) the N - 1 marches", a_march), ("(a) the N - 1 rt_step_kernel launches", a_step), ("(a) kernel total", a_total),
             ("(b) scan march", b_march), ("(b) rt_step_rscan_kernel", b_scan), ("(b) kernel total", b_total),
             ("(c) plain march of N lengths", c[:, 0]), ("(c) plain rt_step_kernel of N lengths", c[:, 1])]
    for what, v in rows:
        say(f"   {what:<40} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
    d_march = np.median(b_march) / np.median(c[:, 0]) - 1.0
    say(f"   scan march against the plain march of N lengths: {100 * d_march:+.2f} % ({np.median(b_march) - np.median(c[:, 0]):+.3f} ms): the boundary stores "
        f"(and no pruning); spread of the block medians {100 * max(spread(b_march), spread(c[:, 0])):.2f} %")
    say(f"   march time saved: (b) {np.median(b_march):.3f} ms against (a) {np.median(a_march):.3f} ms, {100 * (1.0 - np.median(b_march) / np.median(a_march)):+.2f} % "
        f"(predicted from the segments marched: {100 * (1.0 - (N - 1) / (N * (N - 1) / 2)):+.2f} %)")
    say(f"   second pass: one rt_step_rscan_kernel {np.median(b_scan):.3f} ms against the {N - 1} rt_step_kernel {np.median(a_step):.3f} ms "
        f"({100 * (np.median(b_scan) / np.median(a_step) - 1.0):+.2f} %) and against one plain rt_step_kernel of N lengths {np.median(c[:, 1]):.3f} ms "
        f"(x {np.median(b_scan) / np.median(c[:, 1]):.2f})")
    sp_total = max(spread(a_total), spread(b_total))
    gain = 1.0 - np.median(b_total) / np.median(a_total)
    say(f"   kernel total of (b) against (a): {np.median(a_total) - np.median(b_total):+.3f} ms per curve ({100 * gain:+.2f} %), spread of the block medians "
        f"{100 * sp_total:.2f} %: " + ("(b) is faster by more than the spread" if gain > sp_total else "(b) is NOT faster by more than the spread"))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
