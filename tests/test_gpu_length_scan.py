"""The length scan on a plan (rt_hip_plan_enable_length_scan, rt_step_scan_kernel): the step record at every plasma length
n = 2 .. N from ONE forward march.

Inputs (tests/length_scan.py): the seeded-forward problem regrid_seed_beam(seed_small, 9, 5, 6, 5), 1 350 rays, and the
emission-forward problem regrid_beam(ase_forward(ASE_small), 12, 6, 5, 4), 1 440 rays, at N = 6 with the tables repeated
and g0 of length i scaled by 1 + 0.1 i -- no two lengths share a table.  The oracle's census of both is taken in the first
test: rays escape newly at every length from n = 3 on (emission: from n = 2 on), and the exit position of almost every
ray moves from one length to the next, so a kernel that serves a length with the wrong boundary state fails.

Reference for record n, everywhere: the CPU oracle on the PREFIX problem (problem.prefix_lengths: the tables gain[0 .. n)),
reduced by backend.step_outputs_from_image (`reduced` / `gate_step` of tests/test_gpu_step.py), counts from
counts_from_oracle on that problem.  Tiers: TIGHT_TIER seeded and with exact emission, DEFAULT_TIER with the default
emission update.  Against a plain step plan of the prefix problem: "reordering" where the doubles are the same (seeded:
the f64 product sum in slot order; exact emission: ase_update per slot), else the mode's tier -- a prefix plan of n = 3
takes the SF = 6 instance, whose tile-wide choice of the update sees six slots where the scan's is per slot.
The figures are printed before every assertion."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import length_scan as ls
import method_pairs as mp
import seed_profiles as sp
import table_variants as tv
from element_gate import DEFAULT_TIER, TIGHT_TIER, counts_from_oracle
from test_gpu_step import _ray_set, gate_step, reduced

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

KINDS = ["seeded", "emission", "emission_exact"]


# ---------------------------------------------------------------------------------------------- helpers
def problem_of(kind, ase_small, seed_small, N=6):
    return ls.seeded_forward(seed_small, N) if kind == "seeded" else ls.emission_forward(ase_small, N)


def tier_of(kind):
    return DEFAULT_TIER if kind == "emission" else TIGHT_TIER


_refs = {}


def oracle_record(hip, oracle, p, n, rays, key):
    """(reduced oracle outputs of the prefix problem of n lengths, counts, the oracle's own result), computed once."""
    k = (key, n, rays is None)
    if k not in _refs:
        q = ls.prefix(p, n)
        ora = oracle.image_loop(q, q.build_rays() if rays is None else rays)
        _refs[k] = (reduced(hip, q, ora), counts_from_oracle(oracle, q, rays), ora)
    return _refs[k]


def run_scan(plan, rays, exact=False):
    (plan.set_ray_grid() if rays is None else plan.set_rays(rays))
    if exact:
        plan.set_exact_emission(True)
    plan.enable_step().enable_length_scan().run()
    return plan.fetch_length_steps(), plan.fetch()


def plain_step(hip, p, rays, exact=False):
    with hip.Plan(p) as plan:
        (plan.set_ray_grid() if rays is None else plan.set_rays(rays))
        if exact:
            plan.set_exact_emission(True)
        plan.enable_step().run()
        return plan.fetch_step(), plan.fetch()


def gate_records(hip, oracle, p, rays, recs, info, kind, label, key, against_prefix_plan=True):
    assert [r["n"] for r in recs] == list(range(2, p.N + 1))
    full = oracle_record(hip, oracle, p, p.N, rays, key)[2]
    assert info["stats"]["cell_steps"] == full["counters"]["cell_steps"], label      # the march of all N lengths, once
    code = 0
    for rec in recs:
        n = rec["n"]
        ref, counts, ora = oracle_record(hip, oracle, p, n, rays, key)
        print(f"{label} / n = {n}: failure_code {rec['failure_code']} (oracle {ora['failure_code']})")
        assert rec["failure_code"] == ora["failure_code"], (label, n)
        code |= rec["failure_code"]
        q = ls.prefix(p, n)
        gate_step(rec, ref, q, counts, tier_of(kind), f"{label} / n = {n} against the oracle on the prefix problem")
        if against_prefix_plan:
            one, _ = plain_step(hip, q, rays, exact=kind == "emission_exact")
            gate_step(rec, one, q, counts, tier_of(kind) if kind == "emission" else "reordering",
                      f"{label} / n = {n} against a plain step plan of the prefix problem")
    assert info["failure_code"] == code, label


# ---------------------------------------------------------------------------------------------- 0. the census
@pytest.mark.parametrize("kind", ["seeded", "emission"])
def test_census_every_length_has_newly_escaped_rays_and_moved_exits(oracle, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    rays = p.build_rays()
    assert len(rays) == (1350 if kind == "seeded" else 1440) and p.method == 2 and p.N == 6
    for i in range(1, 6):
        for j in range(i + 1, 6):
            assert not np.array_equal(p.gain[i].g0, p.gain[j].g0), (i, j)
    cen = ls.escape_census(oracle, p, rays)
    esc = [int(cen[n][0].sum()) for n in range(2, 7)]
    moved = [int(((cen[n][1]["x"] != cen[n - 1][1]["x"]) | (cen[n][1]["y"] != cen[n - 1][1]["y"])).sum()) for n in range(3, 7)]
    print(f"census / {kind}: escaped at n = 2 .. 6: {esc}; exit position moved from the previous length, n = 3 .. 6: {moved}")
    first = 1 if kind == "seeded" else 0            # (the seeded rays all stay inside the first length)
    assert all(b > a for a, b in zip(esc[first:], esc[first + 1:])) and esc[first + 1] > 0, esc
    if kind == "emission":
        assert esc[0] > 0
    for n in range(3, 7):                            # escaped by n - 1 => escaped by n
        assert not (cen[n - 1][0] & ~cen[n][0]).any()
    assert all(mv >= len(rays) // 2 for mv in moved), moved


# ---------------------------------------------------------------------------------------------- 1. every record against the oracle
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_record_against_the_oracle_and_the_prefix_plans(hip, oracle, ase_small, seed_small, kind, mode):
    p = problem_of(kind, ase_small, seed_small)
    rays = None if mode == "grid" else p.build_rays()
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, rays, exact=kind == "emission_exact")
        assert info["stats"]["n_rays"] == p.n_rays_total and plan.last_fused() is False
        assert plan.last_march_instance() & (8 << 1)                    # the scan instance of the march
        last = plan.fetch_step()            # fetch_step and I_ang of fetch serve record N
        for key in ("E_v", "nf", "I_ang"):
            assert np.array_equal(last[key], recs[-1][key]), key
        assert np.array_equal(info["I_ang"], recs[-1]["I_ang"])
        e, f = plan.step_ptrs()
        assert (e, f) == plan.length_step_ptrs(p.N)[:2]
        views = plan.length_step_tensors()
        assert len(views) == p.N - 1
        for rec, v in zip(recs, views):
            assert v["n"] == rec["n"]
            assert np.array_equal(v["E_v"].cpu().numpy(), rec["E_v"]) and np.array_equal(v["nf"].cpu().numpy().ravel(), rec["nf"])
            assert np.array_equal(v["I_ang"].cpu().numpy().ravel(), rec["I_ang"])
    for a, b in zip(recs, recs[1:]):
        assert a["E_v"].any() and not np.array_equal(a["E_v"], b["E_v"]) and not np.array_equal(a["nf"], b["nf"])
    gate_records(hip, oracle, p, rays, recs, info, kind, f"scan / {kind}, ray {mode}", kind if kind != "emission_exact" else "emission")


# ---------------------------------------------------------------------------------------------- 2. record N, scan on and off
@pytest.mark.parametrize("kind", ["seeded", "emission"])
def test_record_N_is_the_plain_step_record_and_the_scan_switches_off(hip, oracle, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    counts = counts_from_oracle(oracle, p, None)
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_step().run()
        before = plan.fetch_step()
        inst = plan.last_march_instance()
        recs, info = run_scan(plan, None)
        gate_step(recs[-1], before, p, counts, "reordering", f"{kind}: record N of the scan against the same plan's plain step run")
        plan.enable_length_scan(False).run()
        after = plan.fetch_step()
        assert plan.last_march_instance() == inst and plan.fetch_length_steps() == []
        assert plan.hl.lib.rt_hip_plan_fetch_length_step(plan._h, 2, None, None, None, None) == cabi.RT_ERR_ARG
        gate_step(after, before, p, counts, "reordering", f"{kind}: scan off again against the plain step run before it")
        img = plan.enable_step(False).run().fetch()                     # image mode still runs
        assert img["failure_code"] == 0 and img["image"] is not None
        gate_step(reduced(hip, p, img), before, p, counts, "reordering", f"{kind}: image mode after the scan, reduced")


# ---------------------------------------------------------------------------------------------- 3. a failure that depends on the length
@pytest.mark.parametrize("kind", ["seeded", "emission"])
def test_failure_that_depends_on_the_length(hip, oracle, ase_small, seed_small, kind):
    clean = problem_of(kind, ase_small, seed_small)
    p = tv.crafted_nan_lineshape(clean, i=3)          # a NaN in the table of length 3: read by the runs of n >= 4 lengths
    rays = p.build_rays()
    oras = {n: oracle.image_loop(ls.prefix(p, n), rays) for n in range(2, 7)}
    n_fail = {n: len(oras[n]["failed_rays"]) for n in oras}
    print(f"{kind}: oracle failure codes {[oras[n]['failure_code'] for n in oras]}, reported rays {n_fail}")
    assert [oras[n]["failure_code"] for n in (2, 3)] == [0, 0] and all(oras[n]["failure_code"] == 1 << 3 for n in (4, 5, 6))
    assert n_fail[6] == cabi.RT_N_FAILED_MAX             # more failing rays than the report holds
    for mode_rays in (None, rays):
        with hip.Plan(clean) as plan:
            clean_recs, _ = run_scan(plan, mode_rays)
        with hip.Plan(p) as plan:
            recs, info = run_scan(plan, mode_rays)
        assert [r["failure_code"] for r in recs] == [oras[n]["failure_code"] for n in range(2, 7)]
        assert info["failure_code"] == 1 << 3
        # the report: the first RT_N_FAILED_MAX failing rays in list order, what the CPU loop pushes
        assert len(info["failed_rays"]) == cabi.RT_N_FAILED_MAX
        assert [tuple(r) for r in info["failed_rays"].tolist()] == [tuple(r) for r in oras[6]["failed_rays"].tolist()]
        for rec, cl in zip(recs, clean_recs):
            n = rec["n"]
            q = ls.prefix(p, n)
            counts = counts_from_oracle(oracle, q, rays)
            if n <= 3:   # the same tables as the clean problem's: untouched by the repeat
                gate_step(rec, cl, q, counts, "reordering", f"{kind}: record {n} of the failing scan against the clean scan's")
            gate_step(rec, reduced(hip, q, oras[n]), q, counts, tier_of(kind), f"{kind}: record {n} of the failing scan against the oracle")
            assert np.isfinite(rec["E_v"]).all() and np.isfinite(rec["nf"]).all() and np.isfinite(rec["I_ang"]).all()


# ---------------------------------------------------------------------------------------------- 4. other numbers of lengths
@pytest.mark.parametrize("kind", ["seeded", "emission"])
def test_two_records(hip, oracle, ase_small, seed_small, kind):
    """N = 3: one boundary, one chunk; the plain plans of both prefixes take the SF = 6 instances or N = 2."""
    p = problem_of(kind, ase_small, seed_small, N=3)
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, None)
    assert len(recs) == 2
    gate_records(hip, oracle, p, None, recs, info, kind, f"scan / {kind}, N = 3", (kind, 3), against_prefix_plan=kind == "seeded")


def test_ten_lengths_ragged_tile(hip, oracle, seed_small):
    """N = 10 on 450 rays: nine lengths are three chunks (4, 4, 1), the last tile holds two rays."""
    p = ls.scan_problem(sp.e2e_problem(seed_small, "limiter"), 10)
    key = "e2e10"
    if key not in ls._built:
        ls._built[key] = p
    p = ls._built[key]
    assert p.n_rays_total == 450 and p.N == 10
    for rays in (None, p.build_rays()):
        with hip.Plan(p) as plan:
            recs, info = run_scan(plan, rays)
        assert len(recs) == 9 and info["stats"]["n_rays"] == 450
        gate_records(hip, oracle, p, rays, recs, info, "seeded", f"scan / N = 10, 450 rays, {'grid' if rays is None else 'list'}", key,
                     against_prefix_plan=rays is None)


# ---------------------------------------------------------------------------------------------- 5. update_gain
def test_update_gain_keeps_the_scan_on(hip, oracle, ase_small, seed_small):
    p = problem_of("seeded", ase_small, seed_small)
    pb = tv.tables_b(p)
    if "tables_b" not in ls._built:
        ls._built["tables_b"] = pb
    pb = ls._built["tables_b"]
    with hip.Plan(p) as plan:
        recs_a, info_a = run_scan(plan, None)
        plan.update_gain(pb.gain).run()
        recs_b, info_b = plan.fetch_length_steps(), plan.fetch()
    assert len(recs_b) == 5 and not np.array_equal(recs_a[0]["E_v"], recs_b[0]["E_v"])
    gate_records(hip, oracle, p, None, recs_a, info_a, "seeded", "scan before the update", "seeded", against_prefix_plan=False)
    gate_records(hip, oracle, pb, None, recs_b, info_b, "seeded", "scan after update_gain (tables B)", "seeded_b", against_prefix_plan=False)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(hip, ase_small, seed_small):
    lib = hip.HipLibrary.get().lib
    ARG = cabi.RT_ERR_ARG
    six = ls.seeded_forward(seed_small)
    with hip.Plan(mp.seed_backward(six)) as plan:                      # backward plan
        assert lib.rt_hip_plan_enable_length_scan(plan._h, 1) == ARG
        assert b"method" in lib.rt_hip_last_error()
    with hip.Plan(ase_small) as plan:
        assert lib.rt_hip_plan_enable_length_scan(plan._h, 1) == ARG
    with hip.Plan(problem_mod.prefix_lengths(six, 2)) as plan:         # N = 2
        assert lib.rt_hip_plan_enable_length_scan(plan._h, 1) == ARG
        assert lib.rt_hip_plan_enable_length_scan(plan._h, 0) == 0     # (switching off is always accepted)
    with hip.Plan(six) as plan:                                        # with a seed set, both orders
        plan.set_ray_grid().set_seeds([six.seed])
        assert lib.rt_hip_plan_enable_length_scan(plan._h, 1) == ARG
        plan.set_seeds([]).enable_length_scan()
        with pytest.raises(hip.RayTraceError, match="length scan"):
            plan.set_seeds([six.seed])
        # outside step mode, with an I_ang buffer, the other output modes
        with pytest.raises(hip.RayTraceError, match="step mode only"):
            plan.run()
        with pytest.raises(hip.RayTraceError, match="length scan"):
            plan.enable_path()
        with pytest.raises(hip.RayTraceError, match="length scan"):
            plan.enable_spectra()
        plan.enable_step()
        import torch
        buf = torch.zeros(six.beam.na * six.beam.nb + six.beam.nv + six.beam.nx * six.beam.ny + 64, dtype=torch.float64, device="cuda")
        with pytest.raises(hip.RayTraceError, match="no image and no I_ang"):
            plan.run(iang_ptr=buf.data_ptr())
        plan.set_step_buffers(buf.data_ptr(), buf.data_ptr() + 8 * 128)
        with pytest.raises(hip.RayTraceError, match="lent step buffers"):
            plan.run()
        plan.set_step_buffers(0, 0)
        for n in (1, 7, 0, -1):
            plan.set_step_one_launch(True).run()                       # (accepted; the run keeps two kernels)
            assert lib.rt_hip_plan_fetch_length_step(plan._h, n, None, None, None, None) == ARG
            assert lib.rt_hip_plan_length_step_ptrs(plan._h, n, None, None, None) == ARG
        assert plan.last_fused() is False and len(plan.fetch_length_steps()) == 5


# ---------------------------------------------------------------------------------------------- 7. the host-pointer loop
@pytest.mark.parametrize("kind", ["seeded", "emission"])
def test_length_scan_loop_equals_the_plans_records(hip, oracle, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, rays)
    out = hip.length_scan_loop(p, rays)
    assert out["failure_code"] == info["failure_code"] == 0 and len(out["records"]) == 5
    assert out["stats"]["cell_steps"] == info["stats"]["cell_steps"] and out["stats"]["n_rays"] == len(rays)
    for a, b in zip(out["records"], recs):
        assert a["n"] == b["n"] and a["failure_code"] == b["failure_code"]
        q = ls.prefix(p, a["n"])
        gate_step(a, b, q, counts_from_oracle(oracle, q, rays), "reordering", f"{kind}: rt_hip_length_scan_loop record {a['n']} against the plan's")
