"""Step mode as ONE launch (rt_fused_step.hip, rt_hip_plan_set_step_one_launch) against step mode as two kernels (the
march and rt_step_kernel), in one process, on ONE plan, the switch alternating from run to run: device time of a run
from the events (march + frequency pass; the one launch reports (launch, 0)).  A third column: image mode as one launch
(rt_fused.hip) on the same plan and rays -- where the headline comes from.

Shapes: ASE_small; the stand-in (ASE_small x scale_problem(16), 6.384 M rays); the stand-in's 8-way strided shard
(first = 0, stride = 8: one device's share in rt_hip_multi_step_loop).

`blocks` blocks of `runs` alternating runs; per way the block medians and their spread ((max - min) / median) are printed
beside the difference between the ways.  The comparison is inside this process only: no figure from another machine.

  python tools/step_one_launch_ab.py [runs] [blocks] [out]     (this is how profiles/step_one_launch_ab.txt was taken)"""
import importlib
import sys

sys.path.insert(0, '.')
import numpy as np
import torch  # first: one HIP runtime in the process (tests/conftest.py, bench.py)

torch.zeros(1, device="cuda")
rt = importlib.import_module("raytrace-miniapp_amd")
be = importlib.import_module("raytrace-miniapp_amd.backend")

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 24
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else "profiles/step_one_launch_ab.txt"
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def spread(v):
    return (v.max() - v.min()) / np.median(v)


WAYS = ("step, two kernels", "step, one launch", "image, one launch")


def run_way(plan, way):
    if way == 2:
        plan.enable_step(False).run()
    else:
        plan.enable_step(True).set_step_one_launch(way == 1).run()
    assert plan.last_fused() == (way != 0), WAYS[way]
    return plan.kernel_times()


ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
standin = rt.scale_problem(ase, 16.0)
say(f"{runs} runs per block, {blocks} blocks per shape, the three ways alternating within a block; device times from the events, in ms")
for name, p, grid in (("ASE_small", ase, {}), ("stand-in (ASE_small x scale_problem(16))", standin, {}),
                      ("stand-in, 8-way strided shard (first 0, stride 8)", standin, dict(first=0, stride=8))):
    with be.Plan(p) as plan:
        plan.set_ray_grid(**grid)
        for _ in range(3):  # warm-up of the three ways
            for way in range(3):
                run_way(plan, way)
        med = [[], [], []]
        for _ in range(blocks):
            t = [[], [], []]
            for _ in range(runs):
                for way in range(3):
                    t[way].append(run_way(plan, way))
            for way in range(3):
                med[way].append(np.median(np.array(t[way]), axis=0))
        # (not a parity test -- tests/test_gpu_step_one_launch.py gates the elements --: the two step ways left the same record)
        run_way(plan, 0)
        two = plan.fetch_step()
        run_way(plan, 1)
        one = plan.fetch_step()
        assert plan.fetch(want_image=False)["failure_code"] == 0
        for key in ("E_v", "nf", "I_ang"):
            d = np.linalg.norm(one[key] - two[key]) / np.linalg.norm(two[key])
            assert d < 1e-12, (name, key, d)
        n_rays = plan.n_rays
    m = [np.array(v) for v in med]
    total = [v.sum(axis=1) for v in m]
    say(f"\n== {name}: {n_rays} rays, nv {p.beam.nv}")
    for way in range(3):
        say(f"   {WAYS[way]:<20} march {np.median(m[way][:, 0]):8.3f}  freq/step {np.median(m[way][:, 1]):8.3f}  total: median of the block medians "
            f"{np.median(total[way]):8.3f} ms   blocks {' '.join(f'{x:.3f}' for x in total[way])}   spread {100 * spread(total[way]):.2f} %")
    sp = max(spread(total[0]), spread(total[1]))
    gain = 1.0 - np.median(total[1]) / np.median(total[0])
    say(f"   step, one launch against two kernels: {np.median(total[0]) - np.median(total[1]):+.3f} ms per run ({100 * gain:+.2f} %), spread of the block "
        f"medians {100 * sp:.2f} %: " + ("one launch is faster by more than the spread" if gain > sp else
                                         "one launch is slower by more than the spread" if -gain > sp else "no difference beyond the spread"))
    say(f"   step, one launch against image, one launch: {100 * (np.median(total[1]) / np.median(total[2]) - 1.0):+.2f} %")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
