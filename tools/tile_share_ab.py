"""The frequency kernels of this build against the parent commit's, in one process: csrc/librt_hip_prev.so (the parent's
build) and csrc/librt_hip.so alternating run by run on plans of the same problem, kernel times from plan.kernel_times().

Shapes: seed_small, the 6.384 M-ray stand-in, the config-5 shape (1024 x 1024 pixels, nv = 512, one ray per pixel: the
exclusive deposit).  Modes: image mode as two kernels (RT_HIP_FUSED=2: the frequency kernel's time), image mode in one
launch where the plan takes it (the launch's time), spectra mode and step mode (the spectra / step kernel's time).
Per case `blocks` blocks of `runs` alternating runs; the figure of a library is the median of its block medians, the
noise figure is the parent's own spread (max - min) between its block medians, and the new library passes a case when
its median is not above the parent's by more than that spread.

  python tools/tile_share_ab.py [runs] [blocks] [out.txt]        (out.txt: profiles/tile_share_ab.txt)"""
import importlib
import os
import sys

sys.path.insert(0, '.')
import numpy as np

rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
pm = importlib.import_module("raytrace-miniapp_amd.problem")
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 16
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 5
libs = {"prev": be.HipLibrary(be.CSRC / "librt_hip_prev.so"), "new": be.HipLibrary(be.CSRC / "librt_hip.so")}

ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
config5 = pm.regrid_beam(pm.resample_frequency(ase, 512), nx=1024, ny=1024, a_centre=-1.0, b_centre=-4.5)
shapes = (("seed_small", seed, ("image2", "spectra", "step")),
          ("stand-in", rt.scale_problem(ase, 16.0), ("image2", "fused", "spectra", "step")),
          ("config-5 1024^2x512", config5, ("image2", "step")))
lines = [f"{runs} alternating runs per block, {blocks} blocks per case; ms; prev = the parent commit's library, new = this build",
         "time = frequency / spectra / step kernel (image2, spectra, step) or the one launch (fused)",
         f"{'shape':<20} {'mode':<8} {'prev':>8} {'new':>8} {'new/prev-1':>10} {'prev spread':>12} {'new spread':>11}  verdict   block medians prev | new"]
print("\n".join(lines), flush=True)
worst = 0


def set_mode(plan, mode):
    os.environ["RT_HIP_FUSED"] = "1" if mode == "fused" else "2"
    plan.enable_spectra(mode == "spectra")
    plan.enable_step(mode == "step")


for name, p, modes in shapes:
    plans = {k: be.Plan(p, lib=lib) for k, lib in libs.items()}
    for plan in plans.values():
        plan.set_ray_grid()
    for mode in modes:
        col = 0 if mode == "fused" else 1
        for plan in plans.values():  # warm-up
            set_mode(plan, mode)
            for _ in range(3):
                plan.run().kernel_times()
        if any(plan.last_fused() != (mode == "fused") for plan in plans.values()):
            lines.append(f"{name:<20} {mode:<8} not the launch this plan takes: skipped")
            print(lines[-1], flush=True)
            continue
        med = {"prev": [], "new": []}
        for b in range(blocks):
            t = {"prev": [], "new": []}
            for r in range(runs):
                for k in (("prev", "new") if (b + r) % 2 == 0 else ("new", "prev")):  # both orders
                    set_mode(plans[k], mode)
                    t[k].append(plans[k].run().kernel_times()[col])
            for k in t:
                med[k].append(float(np.median(t[k])))
        for plan in plans.values():
            assert plan.fetch(want_image=False)["failure_code"] == 0
        mp, mn = float(np.median(med["prev"])), float(np.median(med["new"]))
        sp, sn = max(med["prev"]) - min(med["prev"]), max(med["new"]) - min(med["new"])
        ok = mn - mp <= sp
        worst += not ok
        lines.append(f"{name:<20} {mode:<8} {mp:8.4f} {mn:8.4f} {100 * (mn / mp - 1):+9.2f}% {sp:12.4f} {sn:11.4f}  "
                     f"{'within ' if ok else 'OUTSIDE'}   {' '.join(f'{x:.4f}' for x in med['prev'])} | {' '.join(f'{x:.4f}' for x in med['new'])}")
        print(lines[-1], flush=True)
    for plan in plans.values():
        plan.close()
lines.append(f"cases outside the parent's own spread: {worst}")
print(lines[-1])
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write("\n".join(lines) + "\n")
