"""calc_ray under TWO seed beams -- per-ray spectra in spectra mode, and at every plasma length n = 2 .. N in length spectra --
two ways, in one process, alternating within a step: device time of the march and of the second pass from the events, on
seed_small's full ray grid, forward and backward (seed_backward).

  (a) two resident single-seed plans, one CREATED with each seed beam, run back to back: two marches that leave the same
      record, two passes that compute the same exp(gl[k]) -- what a caller has on the parent commit.
  (b) one plan created with seed 0 carrying both beams as spectra seeds (rt_hip_plan_set_spectra_seeds): ONE march, one
      rt_spec_seeds_kernel (rt_spec_scan_seeds_kernel) launch that leaves the rows of both seeds.

Spectra mode runs at the file's own N (3: the SF = 6 instances), length spectra at N = 6 (tables repeated and g0 scaled per
length as tests/length_scan.py does it).  Two seed pairs: (own, primed own) -- both beams fill the aperture, every wave needs
the exponential under either seed -- and (own, primed narrow), the pair of the tests, whose second beam lights few rays, so
that most waves of its single-seed plan skip the exponential and way (a) is at its cheapest.

`blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median).  Required on every line:
the kernel total of (b) below that of (a) by more than the spread.  Reported without a threshold: march and pass separately,
the one pass against the two it replaces, and its stores over n_seed L n K 8 bytes.

  python tools/spectra_seeds_ab.py [steps] [blocks] [out]          (this is how profiles/spectra_seeds_ab.txt was taken)"""
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
import length_scan as ls
import method_pairs as mp
import seed_profiles as sp
import seed_scan as sc

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/spectra_seeds_ab.txt"
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
narrow = sc.primed(sp.e2e_problem(seed, "narrow").seed)
say(f"{steps} steps per block, {blocks} blocks per line, the ways alternating within a step; device times from the events, in ms")
say("staging: spectra mode stages the 16 exponentials of a group once and f0_s of a row in its spare doubles, the storing lanes form")
say("(f0_s sfk_s[k]) eg per seed on the way out (128-byte segments); length spectra cut the row into 2 lengths x 2 seeds x 4 frequencies")
say("(32-byte pieces).  RT_SPECTRA_SEEDS_AB_NOTE, where set, names the build that was measured.")
if os.environ.get("RT_SPECTRA_SEEDS_AB_NOTE"):
    say("build: " + os.environ["RT_SPECTRA_SEEDS_AB_NOTE"])
verdicts = []
for mode, N in (("spectra mode", seed.N), ("length spectra", 6)):
    for direction, base in (("forward", seed), ("backward (seed_backward)", mp.seed_backward(seed))):
        p = base if mode == "spectra mode" else ls.scan_problem(base, N)
        L = 1 if mode == "spectra mode" else N - 1
        for pair, second in (("own + primed own", sc.primed(p.seed)), ("own + primed narrow", narrow)):
            seeds = (p.seed, second)
            singles = [be.Plan(sc.with_seed(p, sd, "created with this seed")) for sd in seeds]
            one = be.Plan(p)
            try:
                for plan in singles + [one]:
                    plan.set_ray_grid()
                    (plan.enable_spectra() if mode == "spectra mode" else plan.enable_length_spectra())
                one.set_spectra_seeds(seeds)
                for _ in range(2):  # warm-up of every way
                    for plan in singles + [one]:
                        plan.run()
                        plan.kernel_times()
                med = {"a": [], "b": []}
                for _ in range(blocks):
                    t = {"a": [], "b": []}
                    for _ in range(steps):
                        for plan in singles:
                            plan.run()
                        t["a"].append([x for plan in singles for x in plan.kernel_times()])
                        one.run()
                        t["b"].append(one.kernel_times())
                    for w in t:
                        med[w].append(np.median(np.array(t[w]), axis=0))
                one.fetch(want_image=False)
                # (not a parity test -- tests/test_gpu_spectra_seeds.py gates the rows --: the two ways left the same doubles, on the device)
                views = one.seed_spectra_tensors() if mode == "spectra mode" else one.seed_length_spectra_tensors()
                for s, plan in enumerate(singles):
                    ref = plan.spectra_tensor() if mode == "spectra mode" else plan.length_spectra_tensors()["Iv"]
                    got = views["Iv"][s]
                    for j in range(L):  # (length by length: no second copy of the whole block)
                        x, y = (got, ref) if mode == "spectra mode" else (got[j], ref[j])
                        assert bool(torch.equal(x.view(torch.int64), y.view(torch.int64))), (mode, direction, pair, s, j)
                del views, ref
            finally:
                for plan in singles + [one]:
                    plan.close()
            a, b = np.array(med["a"]), np.array(med["b"])
            a_march, a_pass, a_total = a[:, 0::2].sum(axis=1), a[:, 1::2].sum(axis=1), a.sum(axis=1)
            b_march, b_pass, b_total = b[:, 0], b[:, 1], b.sum(axis=1)
            nbytes = 2 * L * p.n_rays_total * p.beam.nv * 8
            say(f"\n== {mode}, N = {N}, seed_small {direction}, seeds {pair}: {p.n_rays_total} rays, nv {p.beam.nv}, rows of both seeds {nbytes / 1e9:.2f} GB")
            rows = [("(a) the two marches", a_march), ("(a) the two passes", a_pass), ("(a) kernel total", a_total),
                    ("(b) the one march", b_march), ("(b) the one pass", b_pass), ("(b) kernel total", b_total)]
            for what, v in rows:
                say(f"   {what:<24} median of the block medians {np.median(v):9.3f} ms   blocks {' '.join(f'{x:.3f}' for x in v)}   spread {100 * spread(v):.2f} %")
            say(f"   pass: one {np.median(b_pass):.3f} ms against two {np.median(a_pass):.3f} ms, ratio {np.median(b_pass) / np.median(a_pass):.3f}; "
                f"stores {nbytes / np.median(b_pass) / 1e9:.2f} TB/s against {nbytes / np.median(a_pass) / 1e9:.2f} TB/s over n_seed L n K 8 bytes; "
                f"march share of (a) {100 * np.median(a_march) / np.median(a_total):.1f} %")
            sp_total = max(spread(a_total), spread(b_total))
            gain = 1.0 - np.median(b_total) / np.median(a_total)
            ok = gain > sp_total
            verdicts.append(ok)
            say(f"   kernel total: (b) saves {np.median(a_total) - np.median(b_total):.3f} ms of (a) ({100 * gain:.2f} %), spread of the block medians "
                f"{100 * sp_total:.2f} %: " + ("(b) is faster by more than the spread" if ok else "(b) is NOT faster by more than the spread"))
say(f"\nrequired on all {len(verdicts)} lines: " + ("met" if all(verdicts) else f"NOT met ({verdicts.count(False)} lines fail)"))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
