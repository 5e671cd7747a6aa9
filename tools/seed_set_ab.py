"""A step with two seed beams on the same seed-beam grid, two ways, in one process, alternating: device time of the march
and of the frequency pass from the events, on seed_small and on the seed_medium stand-in (seed_small x scale_problem(16)),
in step mode on the ray grid.

  (a) two single-seed step plans run back to back      two marches, two rt_step_kernel launches: what a caller had before
  (b) one plan with the set of both seeds                ONE march, one rt_step_seeds_kernel launch that leaves both records

The second seed is the file's with f[4] reversed in k and f0 x 0.37 (the pair of tests/test_gpu_seed_set.py).  `blocks`
blocks of `steps` steps; per way the block medians and their spread ((max - min) / median) are printed beside the
differences between the ways.  What it has to show: the march of (b) equals the march of ONE plan of (a) within the
spread of the block medians (printed against either plan of (a), and the two against each other: the same kernel on the
same rays), and the kernel total of (b) is below (a)'s by more than that spread.

  python tools/seed_set_ab.py [steps] [blocks] [out]          (this is how profiles/seed_set_ab.txt was taken)"""
import importlib
import sys

sys.path.insert(0, '.')
import numpy as np
import torch  # first: one HIP runtime in the process (tests/conftest.py, bench.py)

torch.zeros(1, device="cuda")
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 24
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/seed_set_ab.txt"
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


def with_seed(p, seed):
    import copy
    q = copy.copy(p)
    q.seed = seed
    return q


seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
say(f"{steps} steps per block, {blocks} blocks per shape, the two ways alternating within a step; device times from the events, in ms")
for name, p in (("seed_small", seed), ("seed_medium stand-in (seed_small x scale_problem(16))", rt.scale_problem(seed, 16.0))):
    s0 = p.seed
    s1 = rt.Seed(list(s0.x), list(s0.f[:4]) + [np.ascontiguousarray(s0.f[4][::-1])], s0.f0 * 0.37)
    with be.Plan(p) as one0, be.Plan(with_seed(p, s1)) as one1, be.Plan(p) as both:
        for plan in (one0, one1, both):
            plan.set_ray_grid().enable_step()
        both.set_seeds([s0, s1])
        for _ in range(3):  # warm-up of both ways
            one0.run()
            one1.run()
            both.run()
            one1.kernel_times(), both.kernel_times()
        # [march of plan 0, freq of plan 0, march of plan 1, freq of plan 1] and [march, freq]
        med = {"a": [], "b": []}
        for _ in range(blocks):
            t = {"a": [], "b": []}
            for _ in range(steps):
                one0.run()
                one1.run()
                t["a"].append(one0.kernel_times() + one1.kernel_times())
                both.run()
                t["b"].append(both.kernel_times())
            for w in ("a", "b"):
                med[w].append(np.median(np.array(t[w]), axis=0))
        recs = both.fetch_seed_steps()
        ref = (one0.fetch_step(), one1.fetch_step())
        assert both.fetch(want_image=False)["failure_code"] == 0
        # (not a parity test -- tests/test_gpu_seed_set.py gates the elements --: the two ways computed the same records)
        for s in range(2):
            for key in ("E_v", "nf", "I_ang"):
                d = np.linalg.norm(recs[s][key] - ref[s][key]) / np.linalg.norm(ref[s][key])
                assert d < 1e-12, (name, s, key, d)
    a, b = np.array(med["a"]), np.array(med["b"])
    a_march1, a_total = a[:, 0], a.sum(axis=1)
    b_march, b_freq, b_total = b[:, 0], b[:, 1], b.sum(axis=1)
    say(f"\n== {name}: {p.n_rays_total} rays, nv {p.beam.nv}")
    for what, v in (("(a) march of ONE plan", a_march1), ("(a) march of the other plan", a[:, 2]), ("(a) rt_step_kernel of one plan", a[:, 1]),
                    ("(a) rt_step_kernel of the other plan", a[:, 3]), ("(a) kernel total of the step", a_total), ("(b) march", b_march),
                    ("(b) rt_step_seeds_kernel", b_freq), ("(b) kernel total of the step", b_total)):
        say(f"   {what:<40} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
    # (the two plans of (a) run the same march kernel on the same rays and tables: their difference is what two plans differ by)
    for which, v in (("one plan", a_march1), ("the other plan", a[:, 2])):
        sp_march = max(spread(v), spread(b_march))
        d_march = np.median(b_march) / np.median(v) - 1.0
        say(f"   march of (b) against the march of {which} of (a): {100 * d_march:+.2f} % ({np.median(b_march) - np.median(v):+.3f} ms), spread of the "
            f"block medians {100 * sp_march:.2f} %: " + ("equal within the spread" if abs(d_march) <= sp_march else "NOT equal within the spread"))
    say(f"   the two marches of (a) against each other: {100 * (np.median(a[:, 2]) / np.median(a_march1) - 1.0):+.2f} %")
    sp_total = max(spread(a_total), spread(b_total))
    gain = 1.0 - np.median(b_total) / np.median(a_total)
    say(f"   kernel total of (b) against (a): {np.median(a_total) - np.median(b_total):+.3f} ms per step ({100 * gain:+.2f} %), spread of the block medians "
        f"{100 * sp_total:.2f} %: " + ("(b) is faster by more than the spread" if gain > sp_total else "(b) is NOT faster by more than the spread"))
    say(f"   frequency pass: one rt_step_seeds_kernel {np.median(b_freq):.3f} ms against two rt_step_kernel "
        f"{np.median(a[:, 1]) + np.median(a[:, 3]):.3f} ms")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
