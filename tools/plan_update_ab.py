"""A time step whose gain tables change, three ways, in one process, alternating: wall time per step around a device
synchronise on the 6.384 M-ray stand-in (ASE_small x scale_problem(16)) and on seed_small, in step mode on the ray grid.

  (a) destroy + create + set_ray_grid + enable_step + run + fetch_step      what a caller had before Plan.update_gain
  (b) update_gain from numpy arrays + run + fetch_step                      the same resident plan
  (c) update_gain from torch tensors on the device + run + fetch_step       the same resident plan, nothing crosses PCIe on the way in

The tables alternate between the file's (A) and tests/table_variants.py's snapshot B from step to step, so every step
really has new tables.  `blocks` blocks of `steps` steps; per way the block medians and their spread ((max - min) / median)
are printed beside the differences between the ways.  Then the device time of the scan and the pack kernel from events
(RT_HIP_TIMING=1 makes rt_hip_plan_update_gain print them; captured here from stderr for a few updates).

  python tools/plan_update_ab.py [steps] [blocks]          (this is how profiles/plan_update.txt was taken)"""
import importlib
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
import torch  # first: one HIP runtime in the process (tests/conftest.py, bench.py)

torch.zeros(1, device="cuda")
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
import table_variants as tv

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 24
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
WAYS = ("a", "b", "c")


def step_recreate(p):
    with be.Plan(p) as plan:
        plan.set_ray_grid().enable_step().run()
        return plan.fetch_step()


def device_times(plan, tables, n=5):
    """[(scan_ms, pack_ms)] of n updates, from the lines rt_hip_plan_update_gain prints under RT_HIP_TIMING"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        os.environ["RT_HIP_TIMING"] = "1"
        try:
            for i in range(n):
                plan.update_gain(tables[i % 2])
        finally:
            del os.environ["RT_HIP_TIMING"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    return [(float(a), float(b)) for a, b in re.findall(r"plan_update scan\s+([\d.]+) ms.*?pack\s+([\d.]+) ms", text)]


def spread(v):
    return (v.max() - v.min()) / np.median(v)


ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
seed = rt.datfile.load('tests/golden/seed_small.dat.xz')
print(f"{steps} steps per block, {blocks} blocks per shape, the three ways alternating within a step; wall time per step in ms around a device synchronise")
for name, p in (("stand-in (ASE_small x scale_problem(16))", rt.scale_problem(ase, 16.0)), ("seed_small", seed)):
    snap = (p, tv.tables_b(p))
    on_dev = [tv.as_tables(q, lambda a: torch.from_numpy(a).to("cuda:0")) for q in snap]
    table_bytes = sum(a.nbytes for g in p.gain[1:] for a in (g.n, g.g0, g.gv) + (() if g.E0 is None else (g.E0,)))
    with be.Plan(p) as plan:
        plan.set_ray_grid().enable_step()
        for w in range(3):  # warm-up of all three
            step_recreate(snap[w % 2])
            plan.update_gain(snap[w % 2]).run().fetch_step()
            plan.update_gain(on_dev[w % 2]).run().fetch_step()
        med = {w: [] for w in WAYS}
        for _ in range(blocks):
            t = {w: [] for w in WAYS}
            for s in range(steps):
                k = s % 2
                for w in WAYS:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if w == "a":
                        step_recreate(snap[k])
                    elif w == "b":
                        plan.update_gain(snap[k]).run().fetch_step()
                    else:
                        plan.update_gain(on_dev[k]).run().fetch_step()
                    torch.cuda.synchronize()
                    t[w].append((time.perf_counter() - t0) * 1e3)
            for w in WAYS:
                med[w].append(np.median(t[w]))
        run_ms = plan.kernel_ms()
        dev = device_times(plan, on_dev)
        assert plan.fetch(want_image=False)["failure_code"] == 0
    m = {w: np.array(med[w]) for w in WAYS}
    print(f"\n== {name}: {p.n_rays_total} rays, tables {table_bytes / 1e6:.2f} MB raw, kernels of a run {run_ms:.3f} ms")
    for w, what in (("a", "(a) destroy + create + set_ray_grid + enable_step"), ("b", "(b) update_gain from numpy"), ("c", "(c) update_gain from torch tensors")):
        print(f"   {what:<52} median of the block medians {np.median(m[w]):8.3f} ms   blocks {' '.join(f'{x:.3f}' for x in m[w])}   spread {100 * spread(m[w]):.2f} %")
    worst = max(spread(m[w]) for w in WAYS)
    for w in ("b", "c"):
        gain = 1.0 - np.median(m[w]) / np.median(m["a"])
        verdict = "faster than (a) by more than the spread" if gain > worst else "NOT faster than (a) by more than the spread"
        print(f"   ({w}) against (a): {np.median(m['a']) - np.median(m[w]):+.3f} ms per step ({100 * gain:+.2f} %), largest spread of a way {100 * worst:.2f} %: {verdict}")
    if dev:
        d = np.array(dev)
        print(f"   device time from events, median of {len(dev)} updates: scan {np.median(d[:, 0]):.4f} ms, pack {np.median(d[:, 1]):.4f} ms")
    else:
        print("   device time from events: not measured (no timing line captured)")
    sys.stdout.flush()
