"""Every kind of run once, at the golden sizes, for a kernel trace: which kernels a library puts on the queue, in which
order and with which grid, work-group and LDS.  Used to show that a change of the launch code (csrc/rt_launch.hip) changed
none of that: run it under the tracer once per library, each run a process of its own, and compare the two lists.

  rocprofv3 --kernel-trace --output-format csv -d <dir>/prev -o trace -- python tools/launch_shapes.py raytrace-miniapp_amd/csrc/librt_hip_prev.so
  rocprofv3 --kernel-trace --output-format csv -d <dir>/new  -o trace -- python tools/launch_shapes.py raytrace-miniapp_amd/csrc/librt_hip.so
  python tools/launch_shapes.py --compare <prev kernel_trace.csv> <new kernel_trace.csv> [out.txt]

(librt_hip_prev.so: the parent commit's build, the convention of tools/tile_share_ab.py.)  The runs: the image loop on
ASE_small and on seed_small (ray lists from the host), a ray-grid run, a spectra run, a step run, a step run in one
launch, a seed-set step run, a path-tracer run."""
import csv
import importlib
import sys

sys.path.insert(0, '.')


def runs(library):
    import numpy as np
    import torch
    if torch.cuda.is_available():      # (one HIP runtime in the process, torch's first: tests/conftest.py)
        torch.zeros(1, device="cuda")
    rt = importlib.import_module("raytrace-miniapp_amd")
    be = importlib.import_module("raytrace-miniapp_amd.backend")
    be.HipLibrary._instance = be.HipLibrary(library)   # image_loop goes through the process-wide library
    ase = rt.datfile.load('tests/golden/ASE_small.dat.xz')
    seed = rt.datfile.load('tests/golden/seed_small.dat.xz')

    def done(what, plan_or_out, fused=None):
        code = plan_or_out["failure_code"] if isinstance(plan_or_out, dict) else plan_or_out.fetch(want_image=False)["failure_code"]
        assert code == 0, (what, code)
        print(f"{what}: ok" + ("" if fused is None else f", one launch: {fused}"), flush=True)

    done("image loop, ASE_small", be.image_loop(ase))
    done("image loop, seed_small", be.image_loop(seed))
    with be.Plan(ase) as plan:
        plan.set_ray_grid().run()
        done("ray grid, ASE_small", plan, plan.last_fused())
        plan.enable_spectra().run()
        done("spectra, ASE_small", plan, plan.last_fused())
        plan.enable_spectra(False).enable_step().run()
        done("step, ASE_small", plan, plan.last_fused())
        plan.set_step_one_launch(True).run()
        done("step in one launch, ASE_small", plan, plan.last_fused())
    with be.Plan(seed) as plan:
        plan.set_ray_grid().run()
        done("ray grid, seed_small", plan, plan.last_fused())
        plan.set_seeds([seed.seed, seed.seed]).enable_step().run()
        done("seed-set step, seed_small", plan, plan.last_fused())
    with be.Plan(ase) as plan:
        got = plan.enable_path().set_rays(ase.build_rays(np.arange(0, 4096, 7))).run().fetch_path()
        print(f"path tracer, ASE_small: ok, {len(got['err'])} rays", flush=True)


def dispatches(path):
    """[(kernel, grid, work-group, LDS bytes)] in dispatch order from a kernel-trace CSV."""
    rows = list(csv.DictReader(open(path, newline="")))

    def col(row, *names):
        for n in names:
            if n in row:
                return row[n]
        raise KeyError(f"{path}: none of {names} among {sorted(row)}")

    rows.sort(key=lambda r: int(col(r, "Dispatch_Id", "Start_Timestamp")))
    out = []
    for r in rows:
        grid = "x".join(col(r, f"Grid_Size_{a}", "Grid_Size") for a in "XYZ") if "Grid_Size_X" in r else col(r, "Grid_Size")
        wg = "x".join(col(r, f"Workgroup_Size_{a}", "Workgroup_Size") for a in "XYZ") if "Workgroup_Size_X" in r else col(r, "Workgroup_Size")
        out.append((col(r, "Kernel_Name"), grid, wg, col(r, "LDS_Block_Size", "LDS_Block_Size_v", "Lds_Block_Size")))
    return out


def compare(prev_csv, new_csv, out_txt=None):
    prev, new = dispatches(prev_csv), dispatches(new_csv)
    same = prev == new
    lines = [f"ordered (kernel, grid, work-group, LDS bytes) of every dispatch; prev = the parent commit's library, new = this build",
             f"prev: {len(prev)} dispatches, new: {len(new)} dispatches -- {'IDENTICAL' if same else 'DIFFERENT'}"]
    for i in range(max(len(prev), len(new))):
        a, b = (prev[i] if i < len(prev) else None), (new[i] if i < len(new) else None)
        if a == b:
            lines.append(f"{i:3d}  both  {a[1]:>12} {a[2]:>10} {a[3]:>7}  {a[0]}")
        else:
            for tag, x in (("PREV", a), ("NEW ", b)):
                if x:
                    lines.append(f"{i:3d}  {tag}  {x[1]:>12} {x[2]:>10} {x[3]:>7}  {x[0]}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_txt:
        open(out_txt, "w").write(text)
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    runs(sys.argv[1])
