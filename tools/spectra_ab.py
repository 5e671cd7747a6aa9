"""Spectra mode (rt_spec_kernel) against image mode as two kernels (the yardstick), in one process, alternating:
march_ms and frequency / spectra kernel ms of both modes on the 6.384 M-ray stand-in and on seed_small, the budget
(freq_ms + n K 8 B / 3.0 TB/s), the achieved store rate, and rt_hip_calc_rays end to end on the stand-in's ray list
with and without the two-buffer overlap.  Run with RT_HIP_FUSED=2 in the environment (the two-kernel image run).

  RT_HIP_FUSED=2 python tools/spectra_ab.py [runs] [kernels-only]          (this is how profiles/spectra_ab.txt was taken)"""
import importlib
import os
import sys

sys.path.insert(0, '.')
import numpy as np

rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 24
assert os.environ.get("RT_HIP_FUSED") == "2", "set RT_HIP_FUSED=2: image mode as two kernels is the yardstick"


def stat(v):
    v = np.asarray(v)
    return f"median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} ms"


ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
for name, p in (("stand-in (ASE_small x scale_problem(16))", rt.scale_problem(ase, 16.0)), ("seed_small", seed)):
    n, K = p.n_rays_total, p.beam.nv
    with be.Plan(p) as plan:
        plan.set_ray_grid()
        for _ in range(3):  # warm-up of both modes
            plan.enable_spectra(False).run().fetch(want_image=False)
            plan.enable_spectra(True).run().fetch()
        t = {False: [], True: []}
        for _ in range(runs):  # alternating
            for mode in (False, True):
                plan.enable_spectra(mode).run()
                assert not plan.last_fused()
                t[mode].append(plan.kernel_times())
        # ... and each mode on its own, back to back: what the march pays for the mode that ran before it
        alone = {}
        for mode in (False, True):
            plan.enable_spectra(mode).run()
            ts = []
            for _ in range(runs):
                plan.run()
                ts.append(plan.kernel_times())
            alone[mode] = np.array(ts)
    im, sp = np.array(t[False]), np.array(t[True])
    out_bytes = n * K * 8
    budget = float(np.median(im[:, 1])) + out_bytes / 3.0e12 * 1e3
    got = float(np.median(sp[:, 1]))
    print(f"== {name}: {n} rays, K = {K}, spectra {out_bytes / 1e9:.3f} GB, {runs} runs each, alternating")
    print(f"   image mode   march {stat(im[:, 0])}   freq    {stat(im[:, 1])}")
    print(f"   spectra mode march {stat(sp[:, 0])}   spectra {stat(sp[:, 1])}")
    print(f"   not alternating: image mode march {stat(alone[False][:, 0])} freq {stat(alone[False][:, 1])}")
    print(f"                  spectra mode march {stat(alone[True][:, 0])} spectra {stat(alone[True][:, 1])}")
    print(f"   budget = image-mode freq_ms + n K 8 B / 3.0 TB/s = {budget:.3f} ms; spectra kernel {got:.3f} ms "
          f"({'within' if got <= budget else 'OVER'} the budget); store rate n K 8 / t = {out_bytes / (got * 1e-3) / 1e12:.2f} TB/s", flush=True)

if "kernels-only" in sys.argv:
    sys.exit(0)
# rt_hip_calc_rays end to end on the stand-in's ray list: host in, host out
p = rt.scale_problem(ase, 16.0)
rays = be.cabi.rays_to_array(p.build_rays())
n, K = len(rays), p.beam.nv
print(f"== rt_hip_calc_rays, {n} rays, host in / host out ({n * K * 8 / 1e9:.3f} GB of spectra)")
for overlap, chunk in (("1", None), ("0", None), ("1", str(1 << 20)), ("0", str(1 << 20))):
    os.environ["RT_HIP_CALC_RAYS_OVERLAP"] = overlap
    if chunk:
        os.environ["RT_HIP_CALC_RAYS_CHUNK"] = chunk
    else:
        os.environ.pop("RT_HIP_CALC_RAYS_CHUNK", None)
    walls, kern = [], []
    for it in range(3):
        out = be.calc_rays(p, rays)
        walls.append(out["stats"]["total_ms"])  # wall time of the C call
        kern.append(out["stats"]["kernel_ms"])
    assert not out["err"].any()
    w, k = min(walls[1:]), float(np.median(kern))
    print(f"   overlap {overlap}, chunk {chunk or 'default (1 GiB of spectra)'}: wall {w:.1f} ms (first call {walls[0]:.1f}), "
          f"kernels {k:.2f} ms = {100 * k / w:.1f} %, everything else (ray conversion, upload, download) {w - k:.1f} ms", flush=True)
