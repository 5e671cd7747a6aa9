"""The suffix scan on a plan (rt_hip_plan_enable_suffix_scan, rt_step_rscan_kernel): the step record of the run of the LAST
n lengths, n = 2 .. N, from ONE backward march.

Inputs (tests/suffix_scan.py): the emission-backward problem regrid_beam(ASE_small, 12, 6, 5, 4), 1 440 rays (22.5 tiles),
and the seeded-backward problem regrid_seed_beam(seed_backward(seed_small), 9, 5, 6, 5), 1 350 rays, at N = 6 with the
tables repeated and g0 of length i scaled by 1 + 0.1 i -- no two lengths share a table.  Their census is asserted in
tests/test_suffix_scan_host.py: rays escape newly in every marched segment (seeded: from the second on), so a kernel that
serves a record with the wrong boundary state, or that starts a suffix at the wrong slot, fails.  Five records are a full
chunk of accumulators and a rest in both instances of the kernel (four and one in emission, three and two gain-only).

Reference for record n, everywhere: the CPU oracle on the SUFFIX problem (problem.suffix_lengths: gain[0] and the last
n - 1 tables), reduced by backend.step_outputs_from_image (`reduced` / `gate_step` of tests/test_gpu_step.py), counts from
counts_from_oracle on that problem.  Tiers: TIGHT_TIER seeded and with exact emission, DEFAULT_TIER with the default
emission update.  Against a plain step plan of the suffix problem: "reordering" seeded (the f64 product sum in slot order)
and with exact emission (ase_update per slot), the tier in emission (a suffix plan of n = 3 takes the SF = 6 instance,
whose tile-wide choice of the update sees six slots where the scan's is per slot).
The figures are printed before every assertion."""
import dataclasses
import importlib

import numpy as np
import pytest

import ase_seeds as A
import length_scan as ls
import method_pairs as mp
import seed_profiles as sp
import suffix_scan as sx
import table_variants as tv
from element_gate import DEFAULT_TIER, TIGHT_TIER, counts_from_oracle
from test_gpu_step import gate_step, reduced

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

KINDS = ["seeded", "emission"]


# ---------------------------------------------------------------------------------------------- helpers
def problem_of(kind, ase_small, seed_small, N=6):
    return sx.seeded_backward(seed_small, N) if kind == "seeded" else sx.emission_backward(ase_small, N)


def tier_of(kind):
    return DEFAULT_TIER if kind == "emission" else TIGHT_TIER


_refs = {}


def oracle_record(hip, oracle, p, n, rays, key):
    """(reduced oracle outputs of the suffix problem of n lengths, counts, the oracle's own result), computed once."""
    k = (key, n, rays is None)
    if k not in _refs:
        q = sx.suffix(p, n)
        ora = oracle.image_loop(q, q.build_rays() if rays is None else rays)
        _refs[k] = (reduced(hip, q, ora), counts_from_oracle(oracle, q, rays), ora)
    return _refs[k]


def run_scan(plan, rays, exact=False):
    (plan.set_ray_grid() if rays is None else plan.set_rays(rays))
    if exact:
        plan.set_exact_emission(True)
    plan.enable_step().enable_suffix_scan().run()
    return plan.fetch_length_steps(), plan.fetch()


def plain_step(hip, p, rays, exact=False):
    with hip.Plan(p) as plan:
        (plan.set_ray_grid() if rays is None else plan.set_rays(rays))
        if exact:
            plan.set_exact_emission(True)
        plan.enable_step().run()
        return plan.fetch_step(), plan.fetch()


def gate_records(hip, oracle, p, rays, recs, info, kind, label, key, against_suffix_plan=True):
    """The scheme of test_gpu_length_scan.gate_records, with the suffix problem for the prefix problem."""
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
        q = sx.suffix(p, n)
        gate_step(rec, ref, q, counts, tier_of(kind), f"{label} / n = {n} against the oracle on the suffix problem")
        if against_suffix_plan:
            one, _ = plain_step(hip, q, rays, exact=kind == "emission_exact")
            gate_step(rec, one, q, counts, tier_of(kind) if kind == "emission" else "reordering",
                      f"{label} / n = {n} against a plain step plan of the suffix problem")
    assert info["failure_code"] == code, label


# ---------------------------------------------------------------------------------------------- 1. every record against the oracle
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_record_against_the_oracle_and_the_suffix_plans(hip, oracle, ase_small, seed_small, kind, mode):
    p = problem_of(kind, ase_small, seed_small)
    rays = None if mode == "grid" else p.build_rays()
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, rays)
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
    gate_records(hip, oracle, p, rays, recs, info, kind, f"suffix scan / {kind}, ray {mode}", kind)


def test_exact_emission(hip, oracle, ase_small, seed_small):
    p = problem_of("emission", ase_small, seed_small)
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, None, exact=True)
    gate_records(hip, oracle, p, None, recs, info, "emission_exact", "suffix scan / exact emission, ray grid", "emission")


# ---------------------------------------------------------------------------------------------- 2. record N, scan on and off
@pytest.mark.parametrize("kind", KINDS)
def test_record_N_is_the_plain_step_record_and_the_scan_switches_off(hip, oracle, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    counts = counts_from_oracle(oracle, p, None)
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_step().run()
        before = plan.fetch_step()
        inst = plan.last_march_instance()
        recs, info = run_scan(plan, None)
        gate_step(recs[-1], before, p, counts, "reordering", f"{kind}: record N of the suffix scan against the same plan's plain step run")
        plan.enable_suffix_scan(False).run()
        after = plan.fetch_step()
        assert plan.last_march_instance() == inst and plan.fetch_length_steps() == []
        assert plan.hl.lib.rt_hip_plan_fetch_length_step(plan._h, 2, None, None, None, None) == cabi.RT_ERR_ARG
        gate_step(after, before, p, counts, "reordering", f"{kind}: scan off again against the plain step run before it")
        img = plan.enable_step(False).run().fetch()                     # image mode still runs
        assert img["failure_code"] == 0 and img["image"] is not None
        gate_step(reduced(hip, p, img), before, p, counts, "reordering", f"{kind}: image mode after the scan, reduced")


# ---------------------------------------------------------------------------------------------- 3. failures that depend on the record
def failing_variant(clean, which):
    """A failing table at length 3 of 5: read by the suffixes of n >= 4 lengths, not by n = 2, 3."""
    if which == "nan":
        return tv.crafted_nan_lineshape(clean, i=3)
    gains = list(clean.gain)        # a negative lineshape table (the negative input of tests/test_gpu_step.py), one length only
    gains[3] = dataclasses.replace(clean.gain[3], gv=-clean.gain[3].gv)
    return tv.with_gain(clean, gains, " negative gv at length 3")


@pytest.mark.parametrize("kind,which", [("seeded", "nan"), ("emission", "nan"), ("emission", "negative")])
def test_failure_that_depends_on_the_record(hip, oracle, ase_small, seed_small, kind, which):
    clean = problem_of(kind, ase_small, seed_small)
    p = failing_variant(clean, which)
    rays = p.build_rays()
    oras = {n: oracle.image_loop(problem_mod.suffix_lengths(p, n), rays) for n in range(2, 7)}
    n_fail = {n: len(oras[n]["failed_rays"]) for n in oras}
    print(f"{kind} / {which}: oracle failure codes {[oras[n]['failure_code'] for n in oras]}, reported rays {n_fail}")
    # NaN: every suffix that reads the table fails with -3, the same rays each time.  Negative: the run that STARTS in the
    # negative length ends below zero (-2); the longer runs amplify what the lengths before it emit and end positive, so the
    # full problem has no failing ray at all -- the report is that of record 4 alone.
    assert [oras[n]["failure_code"] for n in range(2, 7)] == ([0, 0, 8, 8, 8] if which == "nan" else [0, 0, 4, 0, 0])
    failing_n = [n for n in oras if oras[n]["failure_code"]]
    report = [tuple(r) for r in oras[failing_n[0]]["failed_rays"].tolist()]
    assert all([tuple(r) for r in oras[n]["failed_rays"].tolist()] == report for n in failing_n)
    assert len(report) == cabi.RT_N_FAILED_MAX             # more failing rays than the report holds
    for mode_rays in (None, rays):
        with hip.Plan(clean) as plan:
            clean_recs, _ = run_scan(plan, mode_rays)
        with hip.Plan(p) as plan:
            recs, info = run_scan(plan, mode_rays)
        assert [r["failure_code"] for r in recs] == [oras[n]["failure_code"] for n in range(2, 7)]
        assert info["failure_code"] == oras[4]["failure_code"] | oras[5]["failure_code"] | oras[6]["failure_code"]
        # the report: the first RT_N_FAILED_MAX failing rays in list order, what the CPU loop pushes for the failing runs
        # (NaN: the full problem among them)
        assert [tuple(r) for r in info["failed_rays"].tolist()] == report
        for rec, cl in zip(recs, clean_recs):
            n = rec["n"]
            q = sx.suffix(p, n)
            counts = counts_from_oracle(oracle, q, rays)
            if n <= 3:   # the same tables as the clean problem's: untouched by the repeat
                gate_step(rec, cl, q, counts, "reordering", f"{kind} / {which}: record {n} of the failing scan against the clean scan's")
            gate_step(rec, reduced(hip, q, oras[n]), q, counts, tier_of(kind), f"{kind} / {which}: record {n} of the failing scan against the oracle")
            assert np.isfinite(rec["E_v"]).all() and np.isfinite(rec["nf"]).all() and np.isfinite(rec["I_ang"]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_a_steep_list_ray_fails_under_every_record(hip, oracle, ase_small, seed_small, kind):
    """One ray launched almost perpendicular to z (s.z^2 < 0.01, Helper.h:515): error -1 in every suffix run, the ray
    reported once, every record the clean one without it."""
    p = problem_of(kind, ase_small, seed_small)
    bad = p.build_rays().copy()
    bad["a"][7] = 1500.0
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, bad)
    assert [r["failure_code"] for r in recs] == [1 << 1] * 5 and info["failure_code"] == 1 << 1
    assert len(info["failed_rays"]) == 1 and info["failed_rays"][0] == bad[7]
    for rec in recs:
        n = rec["n"]
        q = sx.suffix(p, n)
        ora = oracle.image_loop(q, bad)
        assert ora["failure_code"] == 1 << 1 and len(ora["failed_rays"]) == 1
        gate_step(rec, reduced(hip, q, ora), q, counts_from_oracle(oracle, q, bad), tier_of(kind), f"{kind}: record {n} with a steep ray against the oracle")


# ---------------------------------------------------------------------------------------------- 4. other numbers of lengths
@pytest.mark.parametrize("kind", KINDS)
def test_two_records(hip, oracle, ase_small, seed_small, kind):
    """N = 3: one boundary, less than a chunk; the plain plans of both suffixes take the SF = 6 instances or N = 2."""
    p = problem_of(kind, ase_small, seed_small, N=3)
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, None)
    assert len(recs) == 2
    gate_records(hip, oracle, p, None, recs, info, kind, f"suffix scan / {kind}, N = 3", (kind, 3), against_suffix_plan=kind == "seeded")


def test_ten_lengths_ragged_tile(hip, oracle, seed_small):
    """N = 10 on 450 rays: nine records are three chunks, the last tile holds two rays."""
    key = "e2e10_backward"
    if key not in sx._built:
        sx._built[key] = ls.scan_problem(sp.e2e_problem(mp.seed_backward(seed_small), "limiter"), 10)
    p = sx._built[key]
    assert p.n_rays_total == 450 and p.N == 10 and p.method == 1
    for rays in (None, p.build_rays()):
        with hip.Plan(p) as plan:
            recs, info = run_scan(plan, rays)
        assert len(recs) == 9 and info["stats"]["n_rays"] == 450
        gate_records(hip, oracle, p, rays, recs, info, "seeded", f"suffix scan / N = 10, 450 rays, {'grid' if rays is None else 'list'}", key,
                     against_suffix_plan=rays is None)


# ---------------------------------------------------------------------------------------------- 5. update_gain
@pytest.mark.parametrize("kind", KINDS)
def test_update_gain_keeps_the_scan_on(hip, oracle, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    if (kind, "tables_b") not in sx._built:
        sx._built[(kind, "tables_b")] = tv.tables_b(p)
    pb = sx._built[(kind, "tables_b")]
    with hip.Plan(p) as plan:
        recs_a, info_a = run_scan(plan, None)
        plan.update_gain(pb.gain).run()
        recs_b, info_b = plan.fetch_length_steps(), plan.fetch()
        # a refused update (a non-finite index) leaves the plan and the records of its last run as they were
        with pytest.raises(hip.RayTraceError):
            plan.update_gain(tv.crafted_nan_index(pb, i=2).gain)
        again = plan.fetch_length_steps()
        for a, b in zip(again, recs_b):
            assert all(np.array_equal(a[k], b[k]) for k in ("E_v", "nf", "I_ang")) and a["failure_code"] == b["failure_code"]
        plan.run()
        recs_c = plan.fetch_length_steps()
    assert len(recs_b) == 5 and not np.array_equal(recs_a[0]["E_v"], recs_b[0]["E_v"])
    gate_records(hip, oracle, pb, None, recs_b, info_b, kind, f"{kind}: suffix scan after update_gain (tables B)", (kind, "b"), against_suffix_plan=False)
    for c, b in zip(recs_c, recs_b):
        q = sx.suffix(pb, b["n"])
        gate_step(c, b, q, counts_from_oracle(oracle, q, None), "reordering", f"{kind}: record {b['n']} of the run after the refused update")


# ---------------------------------------------------------------------------------------------- 6. the step history
@pytest.mark.parametrize("kind", KINDS)
def test_history_files_the_records_of_a_suffix_scan(hip, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    with hip.Plan(p) as plan:
        plan.enable_history(2)
        recs, _ = run_scan(plan, None)
        plan.history_append(1)
        hist = plan.fetch_history()
        assert plan.history_info() == dict(n_steps=2, n_rec=5, n_filled=1)
    assert len(hist) == 5
    for rec, h in zip(recs, hist):
        assert list(h["filled"]) == [0, 1]
        for k in ("E_v", "nf", "I_ang"):
            assert np.array_equal(h[k][1], rec[k]) and not h[k][0].any(), (rec["n"], k)
        assert h["failure_code"][1] == rec["failure_code"] == 0


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(hip, ase_small, seed_small):
    import torch

    lib = hip.HipLibrary.get().lib
    ARG = cabi.RT_ERR_ARG

    def refused(rc, *words):
        text = lib.rt_hip_last_error()
        assert rc == ARG and all(w in text for w in words), (rc, text)

    six = sx.emission_backward(ase_small)
    seeded = sx.seeded_backward(seed_small)
    with hip.Plan(ls.seeded_forward(seed_small)) as plan:                       # a forward plan
        refused(lib.rt_hip_plan_enable_suffix_scan(plan._h, 1), b"method")
    with hip.Plan(problem_mod.suffix_lengths(six, 2)) as plan:                  # N = 2
        refused(lib.rt_hip_plan_enable_suffix_scan(plan._h, 1), b"N < 3")
        assert lib.rt_hip_plan_enable_suffix_scan(plan._h, 0) == 0              # (switching off a scan that is off)
    with hip.Plan(mp.seed_backward(ls.seeded_forward(seed_small))) as plan:     # the length scan on a backward plan: as ever
        refused(lib.rt_hip_plan_enable_length_scan(plan._h, 1), b"method")
    with hip.Plan(six) as plan:                                                 # ASE seeds, both orders
        plan.set_ray_grid().enable_step()
        sd = A.seeds_of(six)[0]
        plan.set_ase_seeds([sd])
        refused(lib.rt_hip_plan_enable_suffix_scan(plan._h, 1), b"ASE seeds")
        plan.set_ase_seeds([]).enable_suffix_scan()
        with pytest.raises(hip.RayTraceError, match="suffix scan"):
            plan.set_ase_seeds([sd])
        with pytest.raises(hip.RayTraceError, match="suffix scan"):
            plan.set_scan_ase_seeds([sd])
        refused(lib.rt_hip_plan_enable_length_scan(plan._h, 1), b"method")
        refused(lib.rt_hip_plan_enable_length_scan(plan._h, 0), b"suffix scan")
    with hip.Plan(seeded) as plan:                                              # a seed set, both orders; the other modes
        plan.set_ray_grid().set_seeds([seeded.seed])
        refused(lib.rt_hip_plan_enable_suffix_scan(plan._h, 1), b"seed set")
        plan.set_seeds([]).enable_suffix_scan()
        with pytest.raises(hip.RayTraceError, match="suffix scan"):
            plan.set_seeds([seeded.seed])
        with pytest.raises(hip.RayTraceError, match="suffix scan"):
            plan.set_scan_seeds([seeded.seed])
        with pytest.raises(hip.RayTraceError, match="step mode only"):          # outside step mode
            plan.run()
        with pytest.raises(hip.RayTraceError, match="suffix scan"):
            plan.enable_path()
        with pytest.raises(hip.RayTraceError, match="suffix scan"):
            plan.enable_spectra()
        plan.enable_step()
        b = seeded.beam
        buf = torch.zeros(b.na * b.nb + b.nv + b.nx * b.ny + 64, dtype=torch.float64, device="cuda")
        with pytest.raises(hip.RayTraceError, match="no image and no I_ang"):
            plan.run(iang_ptr=buf.data_ptr())
        plan.set_step_buffers(buf.data_ptr(), buf.data_ptr() + 8 * 128)
        with pytest.raises(hip.RayTraceError, match="lent step buffers"):
            plan.run()
        plan.set_step_buffers(0, 0)
        for n in (1, 7, 0, -1):
            plan.set_step_one_launch(True).run()                                # (accepted; the run keeps two kernels)
            assert lib.rt_hip_plan_fetch_length_step(plan._h, n, None, None, None, None) == ARG
            assert lib.rt_hip_plan_length_step_ptrs(plan._h, n, None, None, None) == ARG
        assert plan.last_fused() is False and len(plan.fetch_length_steps()) == 5


# ---------------------------------------------------------------------------------------------- 8. the host-pointer loop
@pytest.mark.parametrize("kind", KINDS)
def test_suffix_scan_loop_equals_the_plans_records(hip, oracle, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        recs, info = run_scan(plan, rays)
    out = hip.suffix_scan_loop(p, rays)
    assert out["failure_code"] == info["failure_code"] == 0 and len(out["records"]) == 5
    assert out["stats"]["cell_steps"] == info["stats"]["cell_steps"] and out["stats"]["n_rays"] == len(rays)
    for a, b in zip(out["records"], recs):
        assert a["n"] == b["n"] and a["failure_code"] == b["failure_code"]
        q = sx.suffix(p, a["n"])
        gate_step(a, b, q, counts_from_oracle(oracle, q, rays), "reordering", f"{kind}: rt_hip_suffix_scan_loop record {a['n']} against the plan's")


# ---------------------------------------------------------------------------------------------- 9. the probe
@pytest.mark.parametrize("kind", KINDS)
def test_the_probe_is_that_of_the_whole_run(hip, ase_small, seed_small, kind):
    p = problem_of(kind, ase_small, seed_small)
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_probe().enable_step().run()
        plain = plan.fetch_probe()
        plan.enable_suffix_scan().run()
        scan = plan.fetch_probe()
    for key in ("gvl", "evl", "ivl", "ray2", "flags", "steps"):
        assert plain[key].tobytes() == scan[key].tobytes(), key
    assert (plain["flags"] & 1).any() and plain["steps"].any()
