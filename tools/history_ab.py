"""A time loop that keeps every step's records, two ways, in one process on resident plans: wall time per step.

  (a) fetch   update_gain (device tensors) -> run -> fetch_step / fetch_full_step -> host filing (tests/step_history.py:
              file_step)                                   the loop as callers write it without the step history
  (b) append  update_gain (device tensors) -> run -> history_append, ONE fetch_history behind the loop

A loop is `steps` steps; `loops` loops make a block, the two ways alternating loop by loop; per way the block medians of the
wall time per step (loop time / steps, the fetch behind the loop included) and their spread ((max - min) / median) are
printed.  The tables alternate between the file's (A) and tests/table_variants.py's snapshot B.  Then, from events on the
run's stream: the device time of the two history launches, and of one device-to-device copy of the same bytes for scale.

  python tools/history_ab.py [steps] [loops] [blocks]          (this is how profiles/history_ab.txt was taken)"""
import importlib
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
import torch  # first: one HIP runtime in the process (tests/conftest.py, bench.py)

torch.zeros(1, device="cuda")
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")
import ase_seeds as A
import step_history as H
import table_variants as tv

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 16
loops = int(sys.argv[2]) if len(sys.argv) > 2 else 24
blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 3


def spread(v):
    return (v.max() - v.min()) / np.median(v)


def fetch_records(plan, seeded):
    if seeded:
        full = plan.fetch_full_step()
        return [full["ase"]] + full["seeds"]
    rec = plan.fetch_step()
    rec["failure_code"] = 0
    return [rec]


def loop_fetch(plan, tables, seeded, shape):
    hist = H.new_history(steps, *shape)
    for i in range(steps):
        plan.update_gain(tables[i % 2]).run()
        recs = fetch_records(plan, seeded)
        H.file_step(hist, i, recs, [r["failure_code"] for r in recs])
    return hist


def loop_append(plan, tables):
    for i in range(steps):
        plan.update_gain(tables[i % 2]).run().history_append(i)
    return plan.fetch_history()


ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
big = rt.scale_problem(ase, 16.0)
SHAPES = (("ASE_small, its own ray grid, one record", ase, False, {}),
          ("ASE_small, its own ray grid, two ASE seeds (3 records)", ase, True, {}),
          ("stand-in (ASE_small x scale_problem(16)), rays 0, 8, 16 ... of 6.384 M (the shard of one of 8 devices), one record", big, False,
           dict(first=0, stride=8)))
print(f"{steps} steps per loop, {loops} loops per block (the two ways alternating), {blocks} blocks per shape; wall time per step in ms")
for name, p, seeded, grid in SHAPES:
    b = p.beam
    snap = (p, tv.tables_b(p))
    on_dev = [tv.as_tables(q, lambda a: torch.from_numpy(a).to("cuda:0")) for q in snap]
    with be.Plan(p) as plan:
        plan.set_ray_grid(**grid).enable_step()
        if seeded:
            plan.set_ase_seeds([A.wide(p), A.narrow(p)])
        n_rec = 3 if seeded else 1
        shape = (n_rec, b.nv, b.nx * b.ny, b.na * b.nb)
        plan.enable_history(steps)
        for _ in range(2):  # warm-up of both
            loop_fetch(plan, on_dev, seeded, shape)
            loop_append(plan, on_dev)
        med = dict(fetch=[], append=[])
        for _ in range(blocks):
            t = dict(fetch=[], append=[])
            for _ in range(loops):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop_fetch(plan, on_dev, seeded, shape)
                t1 = time.perf_counter()
                loop_append(plan, on_dev)
                t2 = time.perf_counter()
                t["fetch"].append((t1 - t0) * 1e3 / steps)
                t["append"].append((t2 - t1) * 1e3 / steps)
            for w in t:
                med[w].append(float(np.median(t[w])))
        f, a = np.array(med["fetch"]), np.array(med["append"])
        record_bytes = 8 * n_rec * (b.nv + b.nx * b.ny + b.na * b.nb)
        print(f"\n{name}: {plan.n_rays} rays, nv {b.nv}, nx ny {b.nx * b.ny}, na nb {b.na * b.nb}; {record_bytes} bytes of records per step")
        print(f"  (a) fetch + host filing   block medians {np.round(f, 4).tolist()} ms per step, spread {spread(f):.3f}")
        print(f"  (b) history_append        block medians {np.round(a, 4).tolist()} ms per step, spread {spread(a):.3f}")
        print(f"  (a) - (b) = {np.median(f) - np.median(a):+.4f} ms per step ({(np.median(f) - np.median(a)) / np.median(f) * 100:+.1f} % of (a))")
        # device time of the two launches: events on the null stream, where the run and the append are queued
        plan.run()
        torch.cuda.synchronize()
        ms = []
        for i in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            plan.history_append(i % steps)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        src, dst = torch.zeros(record_bytes // 8, dtype=torch.float64, device="cuda"), torch.empty(record_bytes // 8, dtype=torch.float64, device="cuda")
        cp = []
        for i in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            cp.append(e0.elapsed_time(e1))
        print(f"  device time between events around one history_append (two launches): median {np.median(ms) * 1e3:.1f} us, min {min(ms) * 1e3:.1f} us;"
              f" around one device-to-device copy of the same {record_bytes} bytes (torch copy_): median {np.median(cp) * 1e3:.1f} us, min {min(cp) * 1e3:.1f} us")
