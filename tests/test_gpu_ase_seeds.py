"""ASE seeds on an emission plan (rt_hip_plan_set_ase_seeds, rt_step_ase_seeds_kernel): the ASE record and the records of
two seed beams from ONE march.

Inputs: tests/ase_seeds.py -- 1 440 rays of regrid_beam(ASE_small, 12, 6, 5, 4) (22 tiles and a ragged one of 32 rays),
methods 1 and 2, N = 3 (rt_step_ase_seeds_kernel<6>) and N = 5 (<0>), the seeds `wide` and `narrow`; their census is asserted
on the CPU oracle by tests/test_ase_seeds_host.py.

References: record 0 -- oracle.image_loop on the emission problem p, reduced (backend.step_outputs_from_image), and a plain
emission step plan of p; record 1 + s -- the oracle on carry(p, seed s), the same problem created with the seed, whose scale
da db the tests pass as scales[s], and a plain step plan created from it.
Gates (tests/element_gate.py, `gate_step` of tests/test_gpu_step.py): against the oracle's reduced cube TIGHT_TIER for the
seed records and for exact emission, DEFAULT_TIER for default emission; between two device runs "reordering".  The figures
are printed before every assertion (ELEMENT_PARITY_FILE appends them to a file: profiles/ase_seeds_parity.txt)."""
import ctypes as C
import importlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ase_seeds as A
import table_variants as tv
from element_gate import DEFAULT_TIER, TIGHT_TIER, counts_from_oracle
from test_gpu_step import gate_step, reduced

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi
pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- helpers
_refs, _plain = {}, {}


def oracle_record(hip, oracle, q):
    """(reduced oracle outputs, counts, the oracle's own result) of problem q on its ray grid, computed once per problem."""
    if id(q) not in _refs:
        ora = oracle.image_loop(q, q.build_rays())
        _refs[id(q)] = (q, reduced(hip, q, ora), counts_from_oracle(oracle, q, None), ora)
    return _refs[id(q)][1:]


def set_rays(plan, mode):
    return plan.set_ray_grid() if mode == "grid" else plan.set_rays(plan.problem.build_rays())


def plain_step(hip, q, mode, exact=False):
    """(step record, fetch) of a plain step plan of problem q, once per (problem, mode, exact)."""
    key = (id(q), mode, exact)
    if key not in _plain:
        with hip.Plan(q) as plan:
            set_rays(plan, mode).enable_step()
            if exact:
                plan.set_exact_emission(True)
            plan.run()
            _plain[key] = (q, plan.fetch_step(), plan.fetch())
    return _plain[key][1:]


def scales_of(p, seeds):
    return [A.carry(p, s).scale for s in seeds]


def run_full(plan, p, seeds, mode, seeds_first=False):
    if seeds_first:
        plan.set_ase_seeds(seeds, scales_of(p, seeds))
        set_rays(plan, mode)
    else:
        set_rays(plan, mode).set_ase_seeds(seeds, scales_of(p, seeds))
    plan.enable_step().run()
    return plan.fetch_full_step(), plan.fetch()


def gate_record0(hip, oracle, p, rec, mode, tier, label, exact=False):
    ref, counts, ora = oracle_record(hip, oracle, p)
    assert rec["failure_code"] == ora["failure_code"] == 0, label
    gate_step(rec, ref, p, counts, tier, f"{label} / ASE record against the oracle's cube")
    gate_step(rec, plain_step(hip, p, mode, exact)[0], p, counts, "reordering", f"{label} / ASE record against a plain emission step plan")


def gate_seed(hip, oracle, p, seed, rec, mode, label, against_plain=True):
    q = A.carry(p, seed)
    ref, counts, ora = oracle_record(hip, oracle, q)
    assert rec["failure_code"] == ora["failure_code"], label
    gate_step(rec, ref, q, counts, TIGHT_TIER, f"{label} against the oracle on the problem created with the seed")
    if against_plain:
        gate_step(rec, plain_step(hip, q, mode)[0], q, counts, "reordering", f"{label} against a plain step plan created with the seed")


# ---------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("method", [1, 2])
def test_parity_against_the_oracle_and_the_plain_plans(hip, oracle, ase_small, method, mode, N):
    p = A.base(ase_small, method, N)
    seeds = list(A.seeds_of(p))
    label = f"method {method}, ray {mode}, N = {N}"
    with hip.Plan(p) as plan:
        full, info = run_full(plan, p, seeds, mode, seeds_first=(mode == "grid" and N == 5))
        step0 = plan.fetch_step()               # fetch_step and fetch serve record 0
        assert plan.step_ptrs() == plan.full_step_ptrs(0)[:2]
    recs = [full["ase"]] + full["seeds"]
    assert len(full["seeds"]) == 2 and info["failure_code"] == 0 and len(info["failed_rays"]) == 0 and info["stats"]["n_rays"] == 1440
    for key in ("E_v", "nf", "I_ang"):
        assert np.array_equal(step0[key], full["ase"][key]), key
    assert np.array_equal(info["I_ang"], full["ase"]["I_ang"])
    assert info["stats"]["cell_steps"] == oracle_record(hip, oracle, p)[2]["counters"]["cell_steps"]
    assert info["stats"]["cell_steps"] == oracle_record(hip, oracle, A.carry(p, seeds[0]))[2]["counters"]["cell_steps"]
    for rec in recs:
        assert rec["E_v"].any() and rec["nf"].any() and rec["I_ang"].any()          # every record is non-zero
    assert not np.array_equal(recs[1]["E_v"], recs[2]["E_v"]) and not np.array_equal(recs[1]["nf"], recs[2]["nf"])
    assert not np.array_equal(recs[0]["E_v"], recs[1]["E_v"])
    gate_record0(hip, oracle, p, recs[0], mode, DEFAULT_TIER, label)
    for s, seed in enumerate(seeds):
        gate_seed(hip, oracle, p, seed, recs[1 + s], mode, f"{label} / seed {s}")


# ---------------------------------------------------------------------------------------------- 2. the dark variant
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", [1, 2])
def test_rays_with_all_sums_zero_stay_in_the_seed_records(hip, oracle, ase_small, method, N):
    """The emission march marks a ray whose every sum is zero (n_skipped): it is left out of record 0, to which it adds +0,
    and stays in the seed records, where it carries f0_s f_s[4][k] exp(0).  Whole tiles lie in the dark: they skip the emission
    recurrence and run the seed half alone (N = 5: the generic instance's own gain loop)."""
    p = A.base(ase_small, method, N, dark=True)
    seeds = list(A.seeds_of(p))
    label = f"dark, method {method}, N = {N}"
    with hip.Plan(p) as fresh:
        fresh.set_ray_grid().enable_step().enable_probe().run()
        want_probe, want = fresh.fetch_probe(), fresh.fetch()
    with hip.Plan(p) as plan:
        plan.enable_probe()
        full, info = run_full(plan, p, seeds, "grid")
        probe = plan.fetch_probe()
    n_zero = int((~want_probe["gvl"].any(axis=1) & ~want_probe["evl"].any(axis=1)).sum())
    print(f"{label}: n_skipped {info['stats']['n_skipped']}, rays with all sums zero {n_zero}")
    assert info["stats"]["n_skipped"] == want["stats"]["n_skipped"] >= 300
    for key in ("gvl", "evl", "ivl", "flags", "steps"):
        assert np.array_equal(probe[key], want_probe[key]), key
    assert probe["ray2"].tobytes() == want_probe["ray2"].tobytes()
    gate_record0(hip, oracle, p, full["ase"], "grid", DEFAULT_TIER, label)
    for s, seed in enumerate(seeds):
        gate_seed(hip, oracle, p, seed, full["seeds"][s], "grid", f"{label} / seed {s}")
    # (the record of `wide` holds what the >= 300 marked in-range rays carry: without them it misses the oracle by far more
    # than the tier -- tests/test_ase_seeds_host.py asserts that they are there)


# ---------------------------------------------------------------------------------------------- 3. exact emission
@pytest.mark.parametrize("N", [3, 5])
def test_exact_emission(hip, oracle, ase_small, N):
    p = A.base(ase_small, 1, N)
    seeds = list(A.seeds_of(p))
    with hip.Plan(p) as plan:
        plan.set_exact_emission(True)
        full, info = run_full(plan, p, seeds, "grid")
    assert info["failure_code"] == 0
    gate_record0(hip, oracle, p, full["ase"], "grid", TIGHT_TIER, f"exact emission, N = {N}", exact=True)
    for s, seed in enumerate(seeds):
        gate_seed(hip, oracle, p, seed, full["seeds"][s], "grid", f"exact emission, N = {N} / seed {s}", against_plain=False)


# ---------------------------------------------------------------------------------------------- 4. a failing seed
@pytest.mark.parametrize("method,mode", [(1, "list"), (2, "grid")])
def test_a_failing_seed_leaves_the_other_records_alone(hip, oracle, ase_small, method, mode):
    p = A.base(ase_small, method, 3)
    w, n = A.seeds_of(p)
    if ("neg", id(p)) not in _refs:
        _refs[("neg", id(p))] = A.negative(n)
    bad = _refs[("neg", id(p))]
    rays = p.build_rays()
    err = np.asarray(oracle.exit_rays(A.carry(p, bad), rays)[1])
    assert int((err == -2).sum()) > cabi.RT_N_FAILED_MAX and not (err == -1).any()
    with hip.Plan(p) as plan:
        full, info = run_full(plan, p, [w, bad], mode)
        again = plan.fetch_full_step()          # a second fetch serves the repeated run, it does not repeat again
    recs = [full["ase"]] + full["seeds"]
    assert [r["failure_code"] for r in recs] == [0, 0, 1 << 2] and info["failure_code"] == 1 << 2
    for a, b in zip([again["ase"]] + again["seeds"], recs):
        for key in ("E_v", "nf", "I_ang"):
            assert np.array_equal(a[key], b[key]), key
    label = f"failing seed 1, method {method}, ray {mode}"
    gate_record0(hip, oracle, p, recs[0], mode, DEFAULT_TIER, label)
    gate_seed(hip, oracle, p, w, recs[1], mode, f"{label} / seed 0")
    gate_seed(hip, oracle, p, bad, recs[2], mode, f"{label} / seed 1 (the failing rays deposit nothing)", against_plain=False)
    # the report: the first RT_N_FAILED_MAX failing rays in list order, each once
    first = rays[err == -2][:cabi.RT_N_FAILED_MAX]
    assert len(info["failed_rays"]) == cabi.RT_N_FAILED_MAX
    assert info["failed_rays"].tobytes() == first.tobytes()


# ---------------------------------------------------------------------------------------------- 5. lifecycle
_CHILD = r"""
import importlib, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import ase_seeds as A
rt = importlib.import_module("raytrace-miniapp_amd")
hip = importlib.import_module("raytrace-miniapp_amd.backend")
p = A.base(rt.datfile.load(sys.argv[3]), int(sys.argv[4]))
seeds = list(A.seeds_of(p))
def plain():
    with hip.Plan(p) as fresh:
        fresh.set_ray_grid().enable_step().run()
        return fresh.fetch_step()
one, two = plain(), plain()
with hip.Plan(p) as plan:
    plan.set_ray_grid().set_ase_seeds(seeds, [A.carry(p, s).scale for s in seeds]).enable_step().run()
    full = plan.fetch_full_step()
    plan.set_ase_seeds([]).run()
    back = plan.fetch_step()
for key in ("E_v", "nf", "I_ang"):
    assert one[key].any() and full["seeds"][0][key].any(), key
    assert np.array_equal(one[key], two[key]), ("two plain plans", key)
    assert np.array_equal(back[key], one[key]), ("set_ase_seeds([]) against a plain plan", key)
print("SAME BITS")
"""


def test_lifecycle(hip, oracle, ase_small):
    import torch

    p = A.base(ase_small, 2, 3)
    w, n = A.seeds_of(p)
    b = p.beam
    ERR = cabi.RT_ERR_ARG
    if ("tables_b", id(p)) not in _refs:
        _refs[("tables_b", id(p))] = tv.tables_b(p)
    pb = _refs[("tables_b", id(p))]
    keep = []
    two = (cabi.RtSeed * 3)(cabi.seed_record(w, keep), cabi.seed_record(n, keep), cabi.seed_record(w, keep))
    with hip.Plan(p) as plan:
        lib, h = plan.hl.lib, plan._h
        full, info = run_full(plan, p, [w, n], "grid")
        # -- refusals: each RT_ERR_ARG, and the plan keeps working
        assert lib.rt_hip_plan_set_seeds(h, 1, two) == ERR                       # (a seed set needs a seeded plan, as ever)
        assert lib.rt_hip_plan_set_ase_seeds(h, 3, two, None) == ERR
        assert lib.rt_hip_plan_set_ase_seeds(h, -1, two, None) == ERR
        assert lib.rt_hip_plan_set_ase_seeds(h, 2, None, None) == ERR
        short = rt.Seed(list(w.x[:4]) + [w.x[4][:-1].copy()], list(w.f[:4]) + [w.f[4][:-1].copy()], 1.0)
        wrong = (cabi.RtSeed * 2)(cabi.seed_record(w, keep), cabi.seed_record(short, keep))
        assert lib.rt_hip_plan_set_ase_seeds(h, 2, wrong, None) == ERR and b"dim[4]" in lib.rt_hip_last_error()
        assert lib.rt_hip_plan_enable_spectra(h, 1) == ERR and lib.rt_hip_plan_enable_path(h, 1) == ERR
        assert lib.rt_hip_plan_enable_length_scan(h, 1) == ERR
        assert lib.rt_hip_plan_fetch_full_step(h, 3, None, None, None, None) == ERR
        assert lib.rt_hip_plan_full_step_ptrs(h, -1, None, None, None) == ERR
        assert lib.rt_hip_plan_fetch_seed_step(h, 0, None, None, None, None) == ERR   # (not a seed set: the blocks are 1 + n_seed)
        dev = torch.device("cuda", 0)
        ang = torch.zeros(b.na * b.nb + 8, dtype=torch.float64, device=dev)
        assert lib.rt_hip_plan_run(h, None, None, C.c_void_p(ang.data_ptr())) == ERR
        cube = torch.zeros(b.nx * b.ny * b.nv, dtype=torch.float64, device=dev)
        assert lib.rt_hip_plan_run(h, None, C.c_void_p(cube.data_ptr()), None) == ERR
        lent = torch.zeros(b.nv + b.nx * b.ny + 64, dtype=torch.float64, device=dev)
        plan.set_step_buffers(lent.data_ptr(), lent.data_ptr() + 8 * b.nv)
        assert lib.rt_hip_plan_run(h, None, None, None) == ERR and b"lent" in lib.rt_hip_last_error()
        plan.set_step_buffers(0, 0)
        plan.enable_step(False)
        assert lib.rt_hip_plan_run(h, None, None, None) == ERR and b"step mode" in lib.rt_hip_last_error()
        plan.enable_step().set_step_one_launch(True).enable_probe().set_timing_ring(4)     # (one launch: accepted, ignored)
        plan.run()
        assert not plan.last_fused()
        probe, after, info2 = plan.fetch_probe(), plan.fetch_full_step(), plan.fetch()
        assert int(probe["steps"].sum()) == info2["stats"]["cell_steps"]
        march_ms, freq_ms = plan.kernel_times()
        assert march_ms > 0 and freq_ms > 0 and len(plan.ring_times()) == 1
        counts = counts_from_oracle(oracle, p, None)
        gate_step(after["ase"], full["ase"], p, counts, "reordering", "after the refusals / ASE record")
        for s, seed in enumerate((w, n)):
            q = A.carry(p, seed)
            gate_step(after["seeds"][s], full["seeds"][s], q, counts_from_oracle(oracle, q, None), "reordering", f"after the refusals / seed {s}")
        # -- the blocks: 1 + n_seed equal strides inside one allocation; the views read them
        ptrs = [plan.full_step_ptrs(r) for r in range(3)]
        stride = ptrs[1][0] - ptrs[0][0]
        assert stride > 0 and stride % 256 == 0 and all(y - x == stride for a, c in zip(ptrs, ptrs[1:]) for x, y in zip(a, c))
        assert ptrs[0][0] < ptrs[0][1] < ptrs[0][2] < ptrs[1][0] and stride - (ptrs[0][2] - ptrs[0][0]) >= 8 * b.na * b.nb
        views = plan.full_step_tensors()
        torch.cuda.synchronize()
        for view, rec in zip([views["ase"]] + views["seeds"], [after["ase"]] + after["seeds"]):
            assert view["E_v"].shape == (b.nv,) and view["nf"].shape == (b.ny, b.nx) and view["I_ang"].shape == (b.nb, b.na)
            for key in ("E_v", "nf", "I_ang"):
                assert np.array_equal(view[key].cpu().numpy().reshape(-1), rec[key]), key
        # -- update_gain keeps the seeds: the records on the new tables
        plan.set_step_one_launch(False).enable_probe(False)
        plan.update_gain(pb).run()
        new, info3 = plan.fetch_full_step(), plan.fetch()
        assert info3["failure_code"] == 0
        ref, cnt, ora = oracle_record(hip, oracle, pb)
        assert info3["stats"]["cell_steps"] == ora["counters"]["cell_steps"]
        gate_step(new["ase"], ref, pb, cnt, DEFAULT_TIER, "after update_gain / ASE record against the oracle on the new tables")
        for s, seed in enumerate((w, n)):
            q = A.carry(pb, seed)
            ref, cnt, _ = oracle_record(hip, oracle, q)
            gate_step(new["seeds"][s], ref, q, cnt, TIGHT_TIER, f"after update_gain / seed {s} against the oracle on the new tables")
        # -- the seeds removed: a plain emission step plan (here at "reordering"; bit for bit in the serial mode, below)
        plan.update_gain(p).set_ase_seeds([]).run()
        back = plan.fetch_step()
        assert lib.rt_hip_plan_fetch_full_step(h, 0, None, None, None, None) == ERR
        gate_step(back, plain_step(hip, p, "grid")[0], p, counts, "reordering", "seeds removed against a plain emission step plan")
        img = plan.enable_step(False).run().fetch()                  # ... and image mode runs again
        assert img["failure_code"] == 0 and img["image"] is not None
    # a seeded plan, a plan without E0 and a scan plan take no ASE seeds
    one = (cabi.RtSeed * 1)(cabi.seed_record(w, keep))
    with hip.Plan(A.carry(p, w)) as seeded:
        assert seeded.hl.lib.rt_hip_plan_set_ase_seeds(seeded._h, 1, one, None) == ERR
    with hip.Plan(p) as scan:
        scan.enable_step().enable_length_scan()
        assert scan.hl.lib.rt_hip_plan_set_ase_seeds(scan._h, 1, one, None) == ERR
    # bit for bit, RT_HIP_STEP_SERIAL=1 (every step pass as one wave: sums in a fixed order), in a child process
    root = Path(__file__).resolve().parents[1]
    env = dict(os.environ, RT_HIP_STEP_SERIAL="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, str(root), str(root / "tests"), str(root / "tests" / "golden" / "ASE_small.dat.xz"), "2"],
                         env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "SAME BITS" in out.stdout


# ---------------------------------------------------------------------------------------------- 6. the host-pointer loop
@pytest.mark.parametrize("method", [1, 2])
def test_full_step_loop_against_the_plan(hip, oracle, ase_small, method):
    p = A.base(ase_small, method, 3)
    seeds = list(A.seeds_of(p))
    with hip.Plan(p) as plan:
        full, info = run_full(plan, p, seeds, "list")
    out = hip.full_step_loop(p, seeds, scales_of(p, seeds))
    assert out["failure_code"] == 0 and len(out["seeds"]) == 2 and out["stats"]["n_rays"] == 1440 and len(out["failed_rays"]) == 0
    assert out["stats"]["cell_steps"] == info["stats"]["cell_steps"]
    gate_step(out["ase"], full["ase"], p, counts_from_oracle(oracle, p, None), "reordering", f"full_step_loop, method {method} / ASE record")
    for s, seed in enumerate(seeds):
        q = A.carry(p, seed)
        gate_step(out["seeds"][s], full["seeds"][s], q, counts_from_oracle(oracle, q, None), "reordering", f"full_step_loop, method {method} / seed {s}")
    # scales None: the problem's scale for every record
    unscaled = hip.full_step_loop(p, seeds[:1])
    q = A.carry(p, seeds[0])
    assert np.allclose(unscaled["seeds"][0]["nf"] * q.scale, full["seeds"][0]["nf"], rtol=1e-9, atol=0.0)
    assert np.array_equal(unscaled["seeds"][0]["I_ang"].astype(bool), full["seeds"][0]["I_ang"].astype(bool))


# ---------------------------------------------------------------------------------------------- 7. the ray set changes under the seeds
@pytest.mark.parametrize("method", [1, 2])
def test_a_list_behind_a_grid_and_a_grid_behind_a_list_on_one_plan(hip, oracle, ase_small, method):
    """On a forward ray grid the seed factors come from per-seed tables of the grid's points, on a list from seed_factor at the
    launch ray: the ray set of the RUN decides, whatever the plan held before.  The list is the grid's rays reversed -- a
    run that still indexed the grid's tables would give ray t the factor of grid point t, not its own."""
    p = A.base(ase_small, method, 3)
    seeds = list(A.seeds_of(p))
    rays = np.ascontiguousarray(p.build_rays()[::-1])
    with hip.Plan(p) as plan:
        on_grid, _ = run_full(plan, p, seeds, "grid")
        plan.set_rays(rays).run()
        on_list, info = plan.fetch_full_step(), plan.fetch()
        plan.set_ray_grid().run()
        back, info2 = plan.fetch_full_step(), plan.fetch()
    assert info["failure_code"] == info2["failure_code"] == 0 and info["stats"]["n_rays"] == info2["stats"]["n_rays"] == 1440
    for label, full, mode in ((f"method {method}, a list behind a grid", on_list, "list"), (f"method {method}, a grid behind a list", back, "grid")):
        gate_record0(hip, oracle, p, full["ase"], mode, DEFAULT_TIER, label)
        for s, seed in enumerate(seeds):
            # (the same rays in another order: the oracle's reduced cube and the counts per element are those of the grid)
            gate_seed(hip, oracle, p, seed, full["seeds"][s], mode, f"{label} / seed {s}")
    for s in range(2):
        assert on_grid["seeds"][s]["E_v"].any() and on_list["seeds"][s]["E_v"].any()
