"""The whole per-step record -- the ASE triple and the triples of two seed beams -- two ways, in one process, alternating:
device time of the march and of the step pass from the events, on the ASE stand-in (ASE_small x scale_problem(16)) on the
beam's own ray grid, forward (method 2) and backward (method 1), with the seeds `wide` and `narrow` of tests/ase_seeds.py
built for its beam.

  (a) an emission step plan, and a seeded plan of the same problem (carry, tests/ase_seeds.py) with the set of both seeds,
      on the same rays, run back to back       two marches, rt_step_kernel and rt_step_seeds_kernel: what a caller had before
  (b) one emission plan with the ASE seeds     ONE march, one rt_step_ase_seeds_kernel launch that leaves the three records

The baseline is (a) in the same process, never (b) itself.  `blocks` blocks of `steps` steps; per way the block medians and
their spread ((max - min) / median).  What it has to show, or refute:
  1. the march of (b) equals the emission march of (a) within the spread of the block medians;
  2. the pass of (b) lies between the emission pass of (a) alone and the sum of the two passes of (a);
  3. the kernel total of (b) is below (a)'s by about one gain-only march.

  python tools/ase_seeds_ab.py [steps] [blocks] [out]          (this is how profiles/ase_seeds_ab.txt was taken)"""
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
import method_pairs as mp

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/ase_seeds_ab.txt"
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


standin = rt.scale_problem(rt.datfile.load('tests/golden/ASE_small.dat.xz'), 16.0)
say(f"{steps} steps per block, {blocks} blocks per shape, the two ways alternating within a step; device times from the events, in ms")
for name, method in (("forward emission (method 2)", 2), ("backward emission (method 1)", 1)):
    p = mp.with_method(standin, method)
    seeds = [A.wide(p), A.narrow(p)]
    q = A.carry(p, seeds[0])
    scales = [q.scale, q.scale]
    with be.Plan(p) as ase, be.Plan(q) as seeded, be.Plan(p) as full:
        for plan in (ase, seeded, full):
            plan.set_ray_grid().enable_step()
        seeded.set_seeds(seeds)
        full.set_ase_seeds(seeds, scales)
        for _ in range(3):  # warm-up of both ways
            ase.run()
            seeded.run()
            full.run()
            seeded.kernel_times(), full.kernel_times()
        # [emission march, emission pass, gain-only march, seed-set pass] and [march, pass]
        med = {"a": [], "b": []}
        for _ in range(blocks):
            t = {"a": [], "b": []}
            for _ in range(steps):
                ase.run()
                seeded.run()
                t["a"].append(ase.kernel_times() + seeded.kernel_times())
                full.run()
                t["b"].append(full.kernel_times())
            for w in ("a", "b"):
                med[w].append(np.median(np.array(t[w]), axis=0))
        got = full.fetch_full_step()
        ref = [ase.fetch_step()] + seeded.fetch_seed_steps()
        assert full.fetch(want_image=False)["failure_code"] == 0
        # (not a parity test -- tests/test_gpu_ase_seeds.py gates the elements --: the two ways computed the same records)
        for r, rec in enumerate([got["ase"]] + got["seeds"]):
            for key in ("E_v", "nf", "I_ang"):
                d = np.linalg.norm(rec[key] - ref[r][key]) / np.linalg.norm(ref[r][key])
                assert d < 1e-12, (name, r, key, d)
    a, b = np.array(med["a"]), np.array(med["b"])
    a_total, b_total = a.sum(axis=1), b.sum(axis=1)
    say(f"\n== {name}, the stand-in on the beam's own grid: {p.n_rays_total} rays, nv {p.beam.nv}")
    for what, v in (("(a) emission march", a[:, 0]), ("(a) rt_step_kernel (emission)", a[:, 1]), ("(a) gain-only march", a[:, 2]),
                    ("(a) rt_step_seeds_kernel (two seeds)", a[:, 3]), ("(a) kernel total of the step", a_total), ("(b) march", b[:, 0]),
                    ("(b) rt_step_ase_seeds_kernel", b[:, 1]), ("(b) kernel total of the step", b_total)):
        say(f"   {what:<40} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
    m = lambda v: float(np.median(v))
    sp_march = max(spread(a[:, 0]), spread(b[:, 0]))
    d_march = m(b[:, 0]) / m(a[:, 0]) - 1.0
    say(f"   1. march of (b) against the emission march of (a): {100 * d_march:+.2f} % ({m(b[:, 0]) - m(a[:, 0]):+.3f} ms), spread of the block "
        f"medians {100 * sp_march:.2f} %: " + ("equal within the spread" if abs(d_march) <= sp_march else "NOT equal within the spread"))
    lo, hi = m(a[:, 1]), m(a[:, 1]) + m(a[:, 3])
    say(f"   2. pass of (b) {m(b[:, 1]):.3f} ms against the emission pass alone {lo:.3f} ms and the sum of the two passes of (a) {hi:.3f} ms: "
        + ("between the two" if lo <= m(b[:, 1]) <= hi else ("BELOW the emission pass" if m(b[:, 1]) < lo else "ABOVE the sum of the two passes")))
    sp_total = max(spread(a_total), spread(b_total))
    saved = m(a_total) - m(b_total)
    say(f"   3. kernel total of (b) against (a): {-saved:+.3f} ms per step ({-100 * saved / m(a_total):+.2f} %), spread of the block medians "
        f"{100 * sp_total:.2f} %; one gain-only march is {m(a[:, 2]):.3f} ms: the saving is {100 * saved / m(a[:, 2]):.0f} % of it")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
