"""calc_ray at every plasma length n = 2 .. N -- the per-ray side of the gain-length curve -- two ways, in one process,
alternating within a step: device time of the march and of the second pass from the events, on the ray grid, at N = 6
(tables repeated and g0 scaled per length as tests/length_scan.py does it) on the 6.4 M-ray emission stand-ins (ASE_small x
scale_problem(16), backward and forward) and on seed_small's full grid (forward, and backward through seed_backward).

  (a) N - 1 resident spectra-mode plans of the sub-problems (prefix_lengths with the forward method, suffix_lengths with the
      backward one), run back to back: 1 + 2 + ... + (N - 1) plasma segments marched, N - 1 rt_spec_kernel launches --
      what a caller had before.  Their kernels are the parent's (profiles/length_spectra_kernel_resources.txt).
  (b) one plan with length spectra on: ONE scan march of N - 1 segments, one rt_spec_scan_kernel launch that leaves the
      rows of all N - 1 lengths

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  Required: the kernel
total of (b) below that of (a) by more than the spread on all four workloads; the marches alone should drop as the
segments marched predict (-66.7 % at N = 6).  Reported without a threshold: the one pass against the sum of the N - 1
rt_spec_kernel launches, with its bytes per second over L n K 8 -- the figure the staging of rt_spec_scan.hip is judged by --,
and the same pass with 12 and 8 waves per work-group in place of 16 (staging candidate (c) of DESIGN.md 4.18).

  python tools/length_spectra_ab.py [steps] [blocks] [out]          (this is how profiles/length_spectra_ab.txt was taken)"""
import importlib
import os
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

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/length_spectra_ab.txt"
N = 6
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
say(f"N = {N}; {steps} steps per block, {blocks} blocks per workload, the ways alternating within a step; device times from the events, in ms")
big = rt.scale_problem(ase, 16.0)
shapes = (("emission stand-in, backward (ASE_small x scale_problem(16))", ls.scan_problem(big, N)),
          ("emission stand-in, forward (method 2)", ls.scan_problem(mp.ase_forward(big), N)),
          ("seed_small, seeded forward", ls.scan_problem(seed, N)),
          ("seed_small, seeded backward (seed_backward)", ls.scan_problem(mp.seed_backward(seed), N)))
verdicts = []
for name, p in shapes:
    sub = problem_mod.prefix_lengths if p.method == 2 else problem_mod.suffix_lengths
    sub_plans = [be.Plan(sub(p, n)) for n in range(2, N + 1)]
    one = be.Plan(p)
    try:
        for plan in sub_plans:
            plan.set_ray_grid().enable_spectra()
        one.set_ray_grid().enable_length_spectra()
        for _ in range(2):  # warm-up of every way
            for plan in sub_plans + [one]:
                plan.run()
                plan.kernel_times()
        med = {"a": [], "b": []}
        for _ in range(blocks):
            t = {"a": [], "b": []}
            for _ in range(steps):
                for plan in sub_plans:
                    plan.run()
                t["a"].append([x for plan in sub_plans for x in plan.kernel_times()])
                one.run()
                t["b"].append(one.kernel_times())
            for w in t:
                med[w].append(np.median(np.array(t[w]), axis=0))
        assert one.fetch(want_image=False)["failure_code"] == 0
        # (not a parity test -- tests/test_gpu_length_spectra.py gates the rows --: the two ways computed the same spectra, on the device)
        views = one.length_spectra_tensors()
        for j, plan in enumerate(sub_plans):
            ref = plan.spectra_tensor()
            d = float(torch.linalg.norm(views["Iv"][j] - ref) / torch.linalg.norm(ref))
            assert d < 1e-5, (name, j + 2, d)
        del views, ref
        # staging candidate (c), fewer waves per work-group (RT_HIP_FREQ_WG_WAVES applies to this pass): the same kernel and the
        # same staging with 12 and 8 waves per CU, median of the pass over `steps` runs each
        waves_ms = {}
        for nw in (16, 12, 8):
            os.environ["RT_HIP_FREQ_WG_WAVES"] = str(nw)
            one.run()
            one.kernel_times()
            v = []
            for _ in range(steps):
                one.run()
                v.append(one.kernel_times()[1])
            waves_ms[nw] = float(np.median(v))
        del os.environ["RT_HIP_FREQ_WG_WAVES"]
    finally:
        for plan in sub_plans + [one]:
            plan.close()
    a, b = np.array(med["a"]), np.array(med["b"])
    a_march, a_spec, a_total = a[:, 0::2].sum(axis=1), a[:, 1::2].sum(axis=1), a.sum(axis=1)
    b_march, b_pass, b_total = b[:, 0], b[:, 1], b.sum(axis=1)
    nbytes = (N - 1) * p.n_rays_total * p.beam.nv * 8
    say(f"\n== {name}: {p.n_rays_total} rays, nv {p.beam.nv}, rows of all lengths {nbytes / 1e9:.2f} GB")
    rows = [(f"(a) rt_spec_kernel of the plan of n = {n}", a[:, 2 * i + 1]) for i, n in enumerate(range(2, N + 1))]
    rows += [("(a) the N - 1 marches", a_march), ("(a) the N - 1 rt_spec_kernel launches", a_spec), ("(a) kernel total", a_total),
             ("(b) scan march", b_march), ("(b) rt_spec_scan_kernel", b_pass), ("(b) kernel total", b_total)]
    for what, v in rows:
        say(f"   {what:<42} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
    say(f"   march time saved: (b) {np.median(b_march):.3f} ms against (a) {np.median(a_march):.3f} ms, {100 * (1.0 - np.median(b_march) / np.median(a_march)):+.2f} % "
        f"(predicted from the segments marched: {100 * (1.0 - (N - 1) / (N * (N - 1) / 2)):+.2f} %)")
    say(f"   second pass: one rt_spec_scan_kernel {np.median(b_pass):.3f} ms against {N - 1} rt_spec_kernel {np.median(a_spec):.3f} ms, ratio "
        f"{np.median(b_pass) / np.median(a_spec):.3f}; stores {nbytes / np.median(b_pass) / 1e9:.2f} TB/s against {nbytes / np.median(a_spec) / 1e9:.2f} TB/s over L n K 8 bytes")
    say("   rt_spec_scan_kernel with fewer waves per work-group (one work-group per CU): " + ", ".join(f"{nw} waves {ms:.3f} ms" for nw, ms in waves_ms.items()))
    sp_total = max(spread(a_total), spread(b_total))
    gain = 1.0 - np.median(b_total) / np.median(a_total)
    ok = gain > sp_total
    verdicts.append(ok)
    say(f"   kernel total of (b) against (a): {np.median(a_total) - np.median(b_total):+.3f} ms per curve ({100 * gain:+.2f} %), spread of the block medians "
        f"{100 * sp_total:.2f} %: " + ("(b) is faster by more than the spread" if ok else "(b) is NOT faster by more than the spread"))
say(f"\nrequired on all {len(shapes)} workloads: " + ("met" if all(verdicts) else "NOT met"))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
