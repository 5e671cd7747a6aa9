"""The all-devices step entry (rt_hip_multi_step_loop: strided ray grid per device, one sum-reduce of the step record)
against the all-devices image entry (rt_hip_multi_image_loop: pixel-column tiles + gather of the cube), in one process,
alternating, on the 6.384 M-ray stand-in's ray list: wall time per call (host in, host out) at n_devices = 1 -- the real,
degenerate RCCL communicator -- and at loop-back 2 / 4 / 8 (RT_HIP_MULTI_LOOPBACK: n workers on ONE device, the collective
replaced by copies and a sum kernel).  The loop-back rows time the partition, the n plans and the assembly on one device;
they say nothing about n devices or about xGMI.  No number printed here is a gate.

  python tools/multi_step.py [calls]          (this is how profiles/multi_step.txt is taken: output redirected)"""
import importlib
import os
import sys

sys.path.insert(0, '.')
import numpy as np

rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 7

ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
p = rt.scale_problem(ase, 16.0)
rays = p.build_rays()
b = p.beam
record = (b.nv + b.nx * b.ny + b.na * b.nb) * 8
cube = (b.nx * b.ny * b.nv + b.na * b.nb) * 8
print(f"stand-in (ASE_small x scale_problem(16)): {len(rays)} rays as a list; step record {record / 1e6:.3f} MB per device, "
      f"image + I_ang {cube / 1e6:.1f} MB in all")
print(f"{calls} calls of each entry per row, alternating, the first of each dropped; wall time of the C call in ms")
print(f"{'workers':<28} {'entry':<6} {'mode':>4} {'median':>9} {'min':>9} {'max':>9}")
os.environ.pop("RT_HIP_MULTI_LOOPBACK", None)
for label, loop in (("n_devices=1 (RCCL, one rank)", 0), ("loop-back 2", 2), ("loop-back 4", 4), ("loop-back 8", 8)):
    if loop:
        os.environ["RT_HIP_MULTI_LOOPBACK"] = str(loop)
    t = {"image": [], "step": []}
    mode = {}
    for _ in range(calls):
        for name, fn in (("image", be.multi_image_loop), ("step", be.multi_step_loop)):
            out = fn(p, rays, n_devices=1)
            assert out["failure_code"] == 0 and out["stats"]["n_rays"] == len(rays)
            t[name].append(out["call_ms"])
            mode[name] = out["mode"]
    for name in ("image", "step"):
        v = np.array(t[name][1:])
        print(f"{label:<28} {name:<6} {mode[name]:>4} {np.median(v):9.3f} {v.min():9.3f} {v.max():9.3f}", flush=True)
    print(f"{'':<28} step - image (medians): {np.median(t['step'][1:]) - np.median(t['image'][1:]):+.3f} ms per call")
os.environ.pop("RT_HIP_MULTI_LOOPBACK", None)
