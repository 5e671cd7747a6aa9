"""Randomised parity of step mode in one launch (rt_fused_step.hip) against step mode as two kernels, after
tools/fuzz_fused.py: emission-mode problems on the beam's own ray grid -- random grid sizes (any number of rays per
pixel, one ray per pixel excluded: that is the exclusive mode, which keeps two kernels), N = 2 / 3, frequency counts,
gains, sub-ranges and strides of the ray grid -- under random settings of the switches of the one-launch run
(RT_HIP_FUSED_SPLIT, RT_HIP_FUSED_NODES, RT_HIP_FUSED_CONSUMERS, RT_HIP_FUSED_CONSUMERS_FIRST, RT_HIP_LATE_X10).  Every case
runs ONE plan with the switch off and on: the second run must report one launch, the counters and the failure code must
be equal, and E_v, nf and I_ang must pass the "reordering" gate of tests/element_gate.py (gate_step of
tests/test_gpu_step.py), element by element.

A bounded number of cases and one time limit for the whole run: no case is started after `seconds`.

    python tools/fuzz_step_one_launch.py [cases] [seconds] [out]     (this is how profiles/step_one_launch_fuzz.txt was taken)"""
import copy
import importlib
import os
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np

rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
pm = importlib.import_module("raytrace-miniapp_amd.problem")
from element_gate import contribution_counts
from test_gpu_step import gate_step

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 240.0
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/step_one_launch_fuzz.txt"
SWITCHES = {"RT_HIP_FUSED_SPLIT": ("1", "2", "3"), "RT_HIP_FUSED_NODES": ("0", "3", "64"), "RT_HIP_FUSED_CONSUMERS": ("0", "1", "4", "7"),
            "RT_HIP_FUSED_CONSUMERS_FIRST": ("0", "1"), "RT_HIP_LATE_X10": ("0", "32", "1000")}
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


a = rt.datfile.load('tests/golden/ASE_small.dat.xz')
t0 = time.monotonic()
ran = bad = n_one = 0
say(f"step mode, one launch against two kernels: up to {cases} cases, no case started after {seconds:.0f} s")
for seed in range(cases):
    if time.monotonic() - t0 > seconds:
        say(f"time limit reached before case {seed}")
        break
    rng = np.random.default_rng(47000 + seed)
    p = copy.copy(a)
    N = int(rng.integers(2, 4))
    gains = [p.gain[0]]
    for i in range(N - 1):
        g = p.gain[1 + int(rng.integers(0, 2))]
        gains.append(rt.Gain(g.x, g.y, g.n, g.g0 * np.float32(rng.uniform(0.3, 1.5)), g.E0, g.gv, g.Nv))
    p.gain = gains
    if rng.random() < 0.5:
        p = pm.resample_frequency(p, int(rng.choice([3, 5, 18, 33, 52, 64, 66, 100, 130])))
    na, nb = int(rng.integers(2, 20)), int(rng.integers(2, 20))
    big = rng.random() < 0.2                                    # now and then enough rays for every work-group of the device
    nx = int(rng.integers(20, 60)) if big else int(rng.integers(1, 12))
    ny = int(rng.integers(10, 30)) if big else int(rng.integers(1, 8))
    p = pm.regrid_beam(p, nx=nx, ny=ny, na=na, nb=nb)
    total = p.n_rays_total
    kind = int(rng.integers(0, 4))
    first_r, stride = 0, 1
    if kind == 1:
        first_r = int(rng.integers(0, min(total, 500)))
    elif kind == 2:
        stride = int(rng.integers(2, 9))
    count = (total - first_r + stride - 1) // stride
    if kind == 3:
        count = int(rng.integers(1, count + 1))
    env = {k: str(rng.choice(v)) for k, v in SWITCHES.items() if rng.random() < 0.5}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    what = f"case {seed}: N {N} K {p.beam.nv} grid {nx} x {ny} x {na} x {nb} rays {first_r} + {stride} i, i < {count} {env}"
    res = []
    with be.Plan(p) as plan:
        plan.set_ray_grid(first=first_r, stride=stride, count=count).enable_step()
        for on in (False, True):
            plan.set_step_one_launch(on).run()
            out = plan.fetch_step()
            info = plan.fetch()
            res.append((out, info, plan.last_fused()))
    (two, i2, f2), (one, i1, f1) = res
    ran += 1
    n_one += bool(f1)
    lines.append(f"{what}: {'one launch' if f1 else 'two kernels'}")
    counts = contribution_counts(p, p.build_rays(first_r + stride * np.arange(count, dtype=np.int64)))
    try:
        assert not f2 and f1, f"last_fused: {f2} / {f1}"
        assert i1["failure_code"] == i2["failure_code"] == 0, (i1["failure_code"], i2["failure_code"])
        for key in ("n_rays", "cell_steps", "n_escaped", "n_skipped"):
            assert i1["stats"][key] == i2["stats"][key], key
        gate_step(one, two, p, counts, "reordering", what)
    except AssertionError as e:
        bad += 1
        say(f"MISMATCH {what}: {e}")
say(f"cases run {ran} of {cases}, one-launch runs {n_one}, mismatches {bad}, {time.monotonic() - t0:.0f} s")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
