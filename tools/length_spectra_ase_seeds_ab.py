"""calc_ray of an EMISSION problem and of the same problem under TWO seed beams at every plasma length n = 2 .. N -- per-ray
spectra in length spectra mode -- two ways, in one process, alternating within a step: device time of the march and of the second
pass from the events, on the 6.4 M-ray emission stand-in (ASE_small scaled by 16) at N = 6 on the beam's own grid, methods 1 and 2.

  (a) the two resident plans a caller keeps without the feature, run back to back: the emission length-spectra plan, and the
      length-spectra plan of the same problem created with seed a (ase_seeds.carry) carrying both beams as spectra seeds
      (rt_hip_plan_set_spectra_seeds).  Two scan marches that leave the same record and boundary states apart from evl, two passes.
  (b) one emission plan in length spectra with both beams as ASE seeds (rt_hip_plan_set_length_spectra_ase_seeds): ONE scan march,
      one rt_spec_scan_ase_seeds_kernel launch that leaves the ASE curve and the curves of both seeds.

Two seed pairs: (wide, primed wide) -- both beams fill the aperture, every wave needs the exponential under either seed -- and
(wide, narrow), the pair of the tests, whose second beam lights few rays.

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  Expected, not fixed in
advance: the kernel total of (b) below that of (a) by at least one scan march, and the one pass no slower than the two it replaces
by more than the spread.  Also reported: the march of (b) against the emission plan's own scan march (the same instance on the
same rays).  Every line is reported as measured.

  python tools/length_spectra_ase_seeds_ab.py [steps] [blocks] [out]      (this is how profiles/length_spectra_ase_seeds_ab.txt was taken)"""
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
import ase_seeds as A
import length_scan as ls
import method_pairs as mp
import seed_scan as sc

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/length_spectra_ase_seeds_ab.txt"
N = 6
L = N - 1
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


ase = rt.scale_problem(rt.datfile.load('tests/golden/ASE_small.dat.xz'), 16.0)
say(f"N = {N}; {steps} steps per block, {blocks} blocks per line, the ways alternating within a step; device times from the events, in ms")
say("kernel: two walks over the record per tile -- the emission half (the walk of spec_scan_tile<true, BACKWARD>, four lengths per staging), then")
say("the seed half (the walk of spec_scan_seeds_tile<BACKWARD>, two lengths x two seeds per staging, which reads the record and the lineshape rows")
say("again); one [64][XS_ROW] staging per wave.  The whole grid in one run: the three allocations fit beside each other, nothing is sharded.")
say("RT_LENGTH_SPECTRA_ASE_SEEDS_AB_NOTE, where set, names the build that was measured.")
if os.environ.get("RT_LENGTH_SPECTRA_ASE_SEEDS_AB_NOTE"):
    say("build: " + os.environ["RT_LENGTH_SPECTRA_ASE_SEEDS_AB_NOTE"])
verdicts_total, verdicts_pass = [], []
for method in (1, 2):
    p = mp.with_method(ls.scan_problem(mp.with_method(ase, method), N), method)
    wide, narrow = A.wide(p), A.narrow(p)
    for pair, seeds in (("wide + primed wide", (wide, sc.primed(wide))), ("wide + narrow", (wide, narrow))):
        emis, seeded, one = be.Plan(p), be.Plan(A.carry(p, seeds[0])), be.Plan(p)
        two = [emis, seeded]
        try:
            for plan in two + [one]:
                plan.set_ray_grid().enable_length_spectra()
            seeded.set_spectra_seeds(seeds)
            one.set_length_spectra_ase_seeds(seeds)
            for _ in range(2):  # warm-up of every way
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
            one.fetch(want_image=False)
            # (not a parity test -- tests/test_gpu_length_spectra_ase_seeds.py gates the rows --: the two ways left the same doubles, on the device)
            views = one.full_length_spectra_tensors()
            assert bool(torch.equal(views["Iv"][0].view(torch.int64), emis.length_spectra_tensors()["Iv"].view(torch.int64))), (method, pair, "the ASE curve")
            ref = seeded.seed_length_spectra_tensors()["Iv"]
            for s in range(2):
                assert bool(torch.equal(views["Iv"][1 + s].view(torch.int64), ref[s].view(torch.int64))), (method, pair, s)
            del views, ref
        finally:
            for plan in two + [one]:
                plan.close()
        a, b = np.array(med["a"]), np.array(med["b"])
        a_march, a_pass, a_total = a[:, 0::2].sum(axis=1), a[:, 1::2].sum(axis=1), a.sum(axis=1)
        b_march, b_pass, b_total = b[:, 0], b[:, 1], b.sum(axis=1)
        nbytes = 3 * L * p.n_rays_total * p.beam.nv * 8
        say(f"\n== length spectra, method {method}, N = {p.N}, the emission stand-in, seeds {pair}: {p.n_rays_total} rays, nv {p.beam.nv}, rows of the three curves {nbytes / 1e9:.2f} GB")
        rows = [("(a) emission scan march", a[:, 0]), ("(a) seeded scan march", a[:, 2]), ("(a) the two marches", a_march), ("(a) emission pass", a[:, 1]),
                ("(a) two-seed pass", a[:, 3]), ("(a) the two passes", a_pass), ("(a) kernel total", a_total), ("(b) the one march", b_march),
                ("(b) the one pass", b_pass), ("(b) kernel total", b_total)]
        for what, v in rows:
            say(f"   {what:<24} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
        say(f"   march: the one march {np.median(b_march):.3f} ms against the emission plan's own scan march {np.median(a[:, 0]):.3f} ms, the same instance on the same "
            f"rays: {100 * (np.median(b_march) / np.median(a[:, 0]) - 1.0):+.2f} % (spread {100 * max(spread(b_march), spread(a[:, 0])):.2f} %)")
        sp_pass = max(spread(a_pass), spread(b_pass))
        ratio = np.median(b_pass) / np.median(a_pass)
        ok_pass = ratio - 1.0 <= sp_pass
        verdicts_pass.append(ok_pass)
        say(f"   pass: one {np.median(b_pass):.3f} ms against two {np.median(a_pass):.3f} ms, ratio {ratio:.3f}, spread {100 * sp_pass:.2f} %: "
            + ("no slower than the two it replaces by more than the spread" if ok_pass else "SLOWER than the two it replaces by more than the spread")
            + f"; stores {nbytes / np.median(b_pass) / 1e9:.2f} TB/s against {nbytes / np.median(a_pass) / 1e9:.2f} TB/s over 3 L n K 8 bytes; "
            f"march share of (a) {100 * np.median(a_march) / np.median(a_total):.1f} %")
        sp_total = max(spread(a_total), spread(b_total))
        saved = np.median(a_total) - np.median(b_total)
        floor = min(np.median(a[:, 0]), np.median(a[:, 2]))                 # the cheaper of the two scan marches of (a)
        ok = saved >= floor * (1.0 - sp_total)
        verdicts_total.append(ok)
        say(f"   kernel total: (b) saves {saved:.3f} ms of (a) ({100 * saved / np.median(a_total):.2f} %); one scan march of (a) is {floor:.3f} ms, "
            f"spread of the block medians {100 * sp_total:.2f} %: " + ("the run saves at least one scan march" if ok else "the run saves LESS than one scan march"))
say(f"\nexpected on all {len(verdicts_total)} lines, the run saves at least one scan march (within the spread): "
    + ("met" if all(verdicts_total) else f"NOT met ({verdicts_total.count(False)} lines miss)"))
say(f"expected on all {len(verdicts_pass)} lines, the one pass no slower than the two it replaces by more than the spread: "
    + ("met" if all(verdicts_pass) else f"NOT met ({verdicts_pass.count(False)} lines miss)"))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
