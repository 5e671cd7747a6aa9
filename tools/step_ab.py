"""Step mode (rt_step_kernel) against image mode as two kernels (the yardstick), in one process, alternating on the same
plan: march_ms and frequency / step kernel ms of both modes on the 6.384 M-ray stand-in, on seed_small and on the
config-5 shape (1024 x 1024 pixels, nv = 512, one ray per pixel), each as `blocks` repeated blocks of `runs` alternating
runs -- the spread between the block medians of the SAME mode is printed beside the difference between the modes --,
then the wall time per call of rt_hip_step_loop against rt_hip_image_loop on the stand-in's ray list.
Run with RT_HIP_FUSED=2 in the environment (the two-kernel image run).

  RT_HIP_FUSED=2 python tools/step_ab.py [runs] [blocks]          (this is how profiles/step_ab.txt was taken)"""
import importlib
import os
import sys

sys.path.insert(0, '.')
import numpy as np

rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
pm = importlib.import_module("raytrace-miniapp_amd.problem")
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 24
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
assert os.environ.get("RT_HIP_FUSED") == "2", "set RT_HIP_FUSED=2: image mode as two kernels is the yardstick"

ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
config5 = pm.regrid_beam(pm.resample_frequency(ase, 512), nx=1024, ny=1024, a_centre=-1.0, b_centre=-4.5)
cases = (("stand-in (ASE_small x scale_problem(16))", rt.scale_problem(ase, 16.0)), ("seed_small", seed),
         ("config-5 shape 1024^2 x 512, one ray per pixel", config5))
print(f"{runs} alternating runs per block, {blocks} blocks per shape; times are medians over a block, in ms")
print(f"{'shape':<48} {'mode':<6} {'march':>8} {'freq/step':>10}   block medians of freq/step (spread)")
for name, p in cases:
    b = p.beam
    with be.Plan(p) as plan:
        plan.set_ray_grid()
        for _ in range(3):  # warm-up of both modes
            plan.enable_step(False).run().fetch(want_image=False)
            plan.enable_step(True).run().fetch(want_image=False)
        med = {False: [], True: []}
        for _ in range(blocks):
            t = {False: [], True: []}
            for _ in range(runs):  # alternating
                for mode in (False, True):
                    plan.enable_step(mode).run()
                    assert not plan.last_fused()
                    t[mode].append(plan.kernel_times())
            for mode in (False, True):
                med[mode].append(np.median(np.array(t[mode]), axis=0))
        assert plan.fetch(want_image=False)["failure_code"] == 0
    im, st = np.array(med[False]), np.array(med[True])
    f_im, f_st = float(np.median(im[:, 1])), float(np.median(st[:, 1]))

    def spread(v):
        return (v.max() - v.min()) / np.median(v)

    for mode, m in (("image", im), ("step", st)):
        print(f"{name:<48} {mode:<6} {np.median(m[:, 0]):8.3f} {np.median(m[:, 1]):10.3f}   "
              f"{' '.join(f'{x:.3f}' for x in m[:, 1])} ({100 * spread(m[:, 1]):.2f} %)")
    cube = b.nx * b.ny * b.nv * 8
    print(f"{'':<48} step / image = {f_st / f_im:.4f} ({100 * (f_st / f_im - 1):+.2f} %; spread of the image medians "
          f"{100 * spread(im[:, 1]):.2f} %, of the step medians {100 * spread(st[:, 1]):.2f} %); cube not written: {cube / 1e9:.3f} GB, "
          f"{p.n_rays_total} rays", flush=True)

# wall time per call of the two host-pointer entries on the stand-in's ray list (host in, host out)
p = rt.scale_problem(ase, 16.0)
rays = p.build_rays()
calls = {"image": [], "step": []}
for it in range(7):
    calls["image"].append(be.image_loop(p, rays)["call_ms"])
    calls["step"].append(be.step_loop(p, rays)["call_ms"])
print(f"== wall time per call on the stand-in ({len(rays)} rays as a list, image {p.beam.nx * p.beam.ny * p.beam.nv * 8 / 1e6:.1f} MB, "
      f"E_v + nf {(p.beam.nv + p.beam.nx * p.beam.ny) * 8 / 1e3:.1f} KB), 7 calls each, alternating, the first of each dropped")
for k, v in calls.items():
    v = np.array(v[1:])
    print(f"   rt_hip_{k}_loop: median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} ms")
print(f"   difference of the medians: {np.median(calls['image'][1:]) - np.median(calls['step'][1:]):.3f} ms per call")
