"""A seed set on a plan (rt_hip_plan_set_seeds, rt_step_seeds_kernel): the step records of two seed beams from ONE march.

Inputs: seed_profiles.e2e_problem(seed_small, case) -- 450 rays, seven tiles and a ragged one of two rays; the three cases
share beam, seed beam and gains and differ in the Seed only.  They also share one frequency profile, so the second seed of
every pair (written case') gets f[4] reversed in k and f0 x 0.37: a kernel that reads seed 0's f[4] or f0 for seed 1
cannot pass.  `limiter` and `sign` cover the whole seed beam and `narrow` leaves part of the grid out of range on every
axis: every seed of every pair has >= 90 in-range rays (sp.ray_census), and the sets of in-range rays differ between the
seeds of the pair (limiter, narrow') -- they cannot in (sign, limiter'), two profiles that cover the beam, nor in
(narrow, narrow'), one support: there the seeds differ in f[4] and f0, and in the first of the two in the factors.

Reference per seed s: oracle.image_loop on the problem carrying seed s, reduced by backend.step_outputs_from_image
(`reduced` / `gate_step` of tests/test_gpu_step.py); counts from counts_from_oracle on that problem.
Gates: every record against its oracle reduction at TIGHT_TIER, element by element; against a single-seed step plan
created with that seed at "reordering" (two device runs of the same rays: (n_e + K) 2^-52, and an element nothing deposits
into must be exactly 0).  The figures are printed before every assertion (ELEMENT_PARITY_FILE appends them to a file:
profiles/seed_set_parity.txt)."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import method_pairs as mp
import seed_profiles as sp
import table_variants as tv
from element_gate import TIGHT_TIER, counts_from_oracle
from test_gpu_step import _ray_set, gate_step, reduced, same_step_outputs_in_a_failing_run

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

PAIRS = [("limiter", "narrow"), ("sign", "limiter"), ("narrow", "narrow")]


# ---------------------------------------------------------------------------------------------- helpers
def primed(seed):
    """The second seed of a pair: f[4] reversed in k, f0 x 0.37."""
    return rt.Seed(list(seed.x), list(seed.f[:4]) + [np.ascontiguousarray(seed.f[4][::-1])], seed.f0 * 0.37)


def with_seed(p, seed, label):
    q = copy.copy(p)
    q.seed = seed
    q.golden_image = q.golden_I_ang = None
    q.label = f"{p.label} / {label}"
    return q


_problems, _refs = {}, {}


def pair_problems(base, a, b, transform=None, key=""):
    """(problem carrying seed `a`, problem carrying seed `b`'), built once per session (counts_from_oracle keys on identity)."""
    k = (a, b, key)
    if k not in _problems:
        pa, pb = sp.e2e_problem(base, a), sp.e2e_problem(base, b)
        if transform is not None:
            pa, pb = transform(pa), transform(pb)
        _problems[k] = (with_seed(pa, pa.seed, a), with_seed(pb, primed(pb.seed), b + "'"))
    return _problems[k]


def oracle_record(hip, oracle, p, rays, key):
    """(reduced oracle outputs, counts, the oracle's own result) of problem p on rays (None: its ray grid), computed once."""
    if key not in _refs:
        ora = oracle.image_loop(p, p.build_rays() if rays is None else rays)
        _refs[key] = (reduced(hip, p, ora), counts_from_oracle(oracle, p, rays), ora)
    return _refs[key]


def run_set(plan, seeds, rays, first_grid=True):
    if first_grid:
        (plan.set_ray_grid() if rays is None else plan.set_rays(rays)).set_seeds(seeds)
    else:
        plan.set_seeds(seeds)
        plan.set_ray_grid() if rays is None else plan.set_rays(rays)
    plan.enable_step().run()
    return plan.fetch_seed_steps(), plan.fetch()


def single(hip, p, rays):
    """(step record, fetch) of a plain step plan created with p's seed."""
    with hip.Plan(p) as plan:
        (plan.set_ray_grid() if rays is None else plan.set_rays(rays)).enable_step().run()
        return plan.fetch_step(), plan.fetch()


def in_range(seed, rays):
    return np.array([sp.ray_census(seed, rays[i:i + 1])[1] for i in range(len(rays))], dtype=bool)


def gate_pair(hip, oracle, probs, rays, recs, info, label, key, against_single=True):
    assert len(recs) == len(probs)
    for s, (p, rec) in enumerate(zip(probs, recs)):
        ref, counts, ora = oracle_record(hip, oracle, p, rays, (key, s))
        assert rec["failure_code"] == ora["failure_code"], (label, s)
        assert info["stats"]["cell_steps"] == ora["counters"]["cell_steps"], (label, s)
        gate_step(rec, ref, p, counts, TIGHT_TIER, f"{label} / seed {s} against the oracle's cube")
        if against_single:
            one, _ = single(hip, p, rays)
            gate_step(rec, one, p, counts, "reordering", f"{label} / seed {s} against a single-seed step plan")


# ---------------------------------------------------------------------------------------------- 1. pairs against the oracle
@pytest.mark.parametrize("a,b", PAIRS)
@pytest.mark.parametrize("mode", ["grid", "list"])
def test_pairs_against_the_oracle(hip, oracle, seed_small, a, b, mode):
    pa, pb = pair_problems(seed_small, a, b)
    assert pa.n_rays_total == 450
    all_rays = pa.build_rays()
    ina, inb = in_range(pa.seed, all_rays), in_range(pb.seed, all_rays)
    assert ina.sum() >= 90 and inb.sum() >= 90, (int(ina.sum()), int(inb.sum()))
    if sorted((a, b)) == ["limiter", "narrow"]:
        assert not np.array_equal(ina, inb) and (ina & inb).any()
    assert not np.array_equal(pa.seed.f[4], pb.seed.f[4]) and pa.seed.f0 != pb.seed.f0
    rays = None if mode == "grid" else all_rays
    with hip.Plan(pa) as plan:
        recs, info = run_set(plan, [pa.seed, pb.seed], rays)
        assert info["failure_code"] == 0 and len(info["failed_rays"]) == 0 and info["stats"]["n_rays"] == 450
        step0 = plan.fetch_step()        # fetch_step and fetch serve seed 0
        for key in ("E_v", "nf", "I_ang"):
            assert np.array_equal(step0[key], recs[0][key]), key
        assert np.array_equal(info["I_ang"], recs[0]["I_ang"])
    assert not np.array_equal(recs[0]["E_v"], recs[1]["E_v"]) and recs[0]["E_v"].any() and recs[1]["E_v"].any()
    gate_pair(hip, oracle, (pa, pb), rays, recs, info, f"({a}, {b}'), ray {mode}", (a, b, mode))


# ---------------------------------------------------------------------------------------------- 2. set changes
def test_set_changes(hip, oracle, seed_small):
    pa, pb = pair_problems(seed_small, "limiter", "narrow")
    b = pa.beam
    counts = counts_from_oracle(oracle, pa, None)
    plain, _ = single(hip, pa, None)
    with hip.Plan(pa) as plan:
        # n_seed = 1 with the creation seed: the record of the plain step plan
        recs, info = run_set(plan, [pa.seed], None)
        assert len(recs) == 1 and info["failure_code"] == 0
        gate_step(recs[0], plain, pa, counts, "reordering", "n_seed = 1 with the creation seed against the plain step plan")
        # the set removed: plain step mode, and image mode still runs
        plan.set_seeds([]).run()
        back = plan.fetch_step()
        assert plan.fetch_seed_steps() == []
        assert plan.hl.lib.rt_hip_plan_fetch_seed_step(plan._h, 0, None, None, None, None) == cabi.RT_ERR_ARG
        gate_step(back, plain, pa, counts, "reordering", "set removed: plain step mode against a fresh plan")
        img = plan.enable_step(False).run().fetch()
        assert img["failure_code"] == 0 and img["image"] is not None
        gate_step(reduced(hip, pa, img), plain, pa, counts, "reordering", "set removed: image mode, reduced, against the step plan")
        # both orders of set_ray_grid and set_seeds
        first, _ = run_set(plan, [pa.seed, pb.seed], None, first_grid=True)
    with hip.Plan(pa) as plan:
        second, _ = run_set(plan, [pa.seed, pb.seed], None, first_grid=False)
        for s, p in enumerate((pa, pb)):
            gate_step(second[s], first[s], p, counts_from_oracle(oracle, p, None), "reordering", f"set_seeds before set_ray_grid / seed {s}")
        # a second set with other dim[0..3] replaces the first
        qa, qb = pair_problems(seed_small, "sign", "limiter")
        dims = lambda seeds: [[len(v) for v in sd.x[:4]] for sd in seeds]
        assert dims([qb.seed, qa.seed]) != dims([pa.seed, pb.seed])
        plan.set_seeds([qb.seed, qa.seed]).run()
        recs = plan.fetch_seed_steps()
        info = plan.fetch()
    for s, p in enumerate((qb, qa)):
        ref, cnt, ora = oracle_record(hip, oracle, p, None, (("sign", "limiter", "grid"), 1 - s))
        gate_step(recs[s], ref, p, cnt, TIGHT_TIER, f"replaced set / seed {s} against the oracle's cube")
    assert b.nv == len(recs[0]["E_v"])


# ---------------------------------------------------------------------------------------------- 3. generic instance
def test_generic_instance_five_lengths(hip, oracle, seed_small):
    """N = 5 takes rt_step_seeds_kernel<0>; gains repeated as test_other_numbers_of_lengths repeats them; a ray list."""
    def five(p):
        q = copy.copy(p)
        g = p.gain
        q.gain = [g[0]] + [g[1 + (i % 2)] for i in range(4)]
        return q

    pa, pb = pair_problems(seed_small, "limiter", "narrow", five, "N5")
    assert len(pa.gain) == 5
    rays = pa.build_rays()
    with hip.Plan(pa) as plan:
        recs, info = run_set(plan, [pa.seed, pb.seed], rays)
    assert info["failure_code"] == 0
    gate_pair(hip, oracle, (pa, pb), rays, recs, info, "N = 5, (limiter, narrow'), ray list", ("N5", "list"))


def test_backward_method(hip, oracle, seed_small):
    """Method 1 on a seeded plan: the seed factor is seed_factor at the EXIT ray (Helper.h:523-533), per seed; the deposit
    is at the launch ray.  A ray list (the counts of a whole grid in method 1 assume the beam's own grid)."""
    def backward(p):
        return mp.with_method(p, 1)      # (Problem.method follows the seed; the C ABI takes any pair)

    pa, pb = pair_problems(seed_small, "limiter", "narrow", backward, "method1")
    assert pa.method == 1 and pb.method == 1
    rays = pa.build_rays()
    with hip.Plan(pa) as plan:
        recs, info = run_set(plan, [pa.seed, pb.seed], rays)
    assert info["failure_code"] == 0 and recs[0]["E_v"].any() and recs[1]["E_v"].any()
    gate_pair(hip, oracle, (pa, pb), rays, recs, info, "method 1, (limiter, narrow'), ray list", ("method1", "list"))


# ---------------------------------------------------------------------------------------------- 4. more frequencies
def test_frequency_count_that_is_no_multiple_of_four(hip, oracle, seed_small):
    """nv = 130 (seed_small has 82, Kp = 84): two padding columns in each of the two E_v accumulators, more frequencies
    than the 64 lanes of a flush pass."""
    base = problem_mod.resample_frequency(seed_small, 130)
    pa, pb = pair_problems(base, "sign", "narrow", None, "nv130")
    assert pa.beam.nv == 130 and len(pb.seed.f[4]) == 130
    with hip.Plan(pa) as plan:
        recs, info = run_set(plan, [pa.seed, pb.seed], None)
    assert info["failure_code"] == 0
    gate_pair(hip, oracle, (pa, pb), None, recs, info, "nv = 130, (sign, narrow'), ray grid", ("nv130", "grid"))


# ---------------------------------------------------------------------------------------------- 5. failures per seed
def test_failures_per_seed(hip, oracle, seed_small):
    pl, pb = pair_problems(seed_small, "limiter", "narrow")
    f4 = pl.seed.f[4].copy()
    f4[1] = -abs(f4[1])
    pa = with_seed(pl, rt.Seed(list(pl.seed.x), list(pl.seed.f[:4]) + [f4], pl.seed.f0), "limiter, f[4][1] negative")
    rays = pa.build_rays()
    ora = oracle.image_loop(pa, rays)
    err = np.asarray(oracle.exit_rays(pa, rays)[1])
    print(f"seed A: oracle failure code {ora['failure_code']}, rays with error -2: {int((err == -2).sum())} of {len(rays)}")
    assert ora["failure_code"] == 1 << 2 and int((err == -2).sum()) > 32 and not (err == -1).any()
    one, one_info = single(hip, pa, None)
    assert one_info["failure_code"] == 1 << 2 and len(one_info["failed_rays"]) == 32
    with hip.Plan(pl) as plan:
        recs, info = run_set(plan, [pa.seed, pb.seed], None)
        assert [r["failure_code"] for r in recs] == [1 << 2, 0]
        assert info["failure_code"] == 1 << 2
        assert _ray_set(info["failed_rays"]) == _ray_set(one_info["failed_rays"])
        again = plan.fetch_seed_steps()      # a second fetch serves the repeated run, it does not repeat again
        for key in ("E_v", "nf", "I_ang"):
            assert np.array_equal(again[0][key], recs[0][key]) and np.array_equal(again[1][key], recs[1][key]), key
    ref_b, counts_b, _ = oracle_record(hip, oracle, pb, None, (("limiter", "narrow", "grid"), 1))
    gate_step(recs[1], ref_b, pb, counts_b, TIGHT_TIER, "seed B beside a failing seed A, against the oracle's cube")
    same_step_outputs_in_a_failing_run(recs[0], reduced(hip, pa, ora))
    same_step_outputs_in_a_failing_run(recs[0], one)

    # error -1 does not depend on the seed: a list with one invalid ray
    bad = pl.build_rays()
    bad["a"][7] = 1500.0
    with hip.Plan(pl) as plan:
        recs, info = run_set(plan, [pl.seed, pb.seed], bad)
    assert [r["failure_code"] for r in recs] == [1 << 1, 1 << 1] and info["failure_code"] == 1 << 1
    assert len(info["failed_rays"]) == 1 and info["failed_rays"][0] == bad[7]
    for s, p in enumerate((pl, pb)):
        o = oracle.image_loop(p, bad)
        assert o["failure_code"] == 1 << 1
        gate_step(recs[s], reduced(hip, p, o), p, counts_from_oracle(oracle, p, bad), TIGHT_TIER,
                  f"one invalid ray / seed {s} against the oracle's cube")


# ---------------------------------------------------------------------------------------------- 6. update keeps the set
def test_update_gain_keeps_the_set(hip, oracle, seed_small):
    pa, pb = pair_problems(seed_small, "limiter", "narrow")
    na, nb_ = tv.tables_b(pa), tv.tables_b(pb)
    with hip.Plan(pa) as plan:
        recs, info = run_set(plan, [pa.seed, pb.seed], None)
        plan.update_gain(na).run()
        recs = plan.fetch_seed_steps()
        info = plan.fetch()
        flags = plan.table_flags()
    with hip.Plan(na) as fresh:
        want = fresh.table_flags()
    assert flags["bounded"] == want["bounded"] and flags["ntest_proven"] == want["ntest_proven"]
    assert flags["gv_nonfinite"] == want["gv_nonfinite"] and flags["gs_cap"].tobytes() == want["gs_cap"].tobytes()
    assert info["failure_code"] == 0
    for s, p in enumerate((na, nb_)):
        o = oracle.image_loop(p, p.build_rays())
        assert info["stats"]["cell_steps"] == o["counters"]["cell_steps"]
        gate_step(recs[s], reduced(hip, p, o), p, counts_from_oracle(oracle, p, None), TIGHT_TIER,
                  f"after update_gain / seed {s} against the oracle on the new tables")


# ---------------------------------------------------------------------------------------------- 7. contract
def test_contract(hip, oracle, seed_small, ase_small):
    import torch

    pa, pb = pair_problems(seed_small, "limiter", "narrow")
    b = pa.beam
    keep = []
    two = (cabi.RtSeed * 3)(cabi.seed_record(pa.seed, keep), cabi.seed_record(pb.seed, keep), cabi.seed_record(pa.seed, keep))
    ERR = cabi.RT_ERR_ARG
    # a plan created without a seed takes no set
    q = problem_mod.regrid_beam(ase_small, nx=4, ny=3, na=3, nb=3)
    assert q.seed is None
    with hip.Plan(q) as plan:
        three = (cabi.RtSeed * 1)(cabi.seed_record(pa.seed, keep))
        assert plan.hl.lib.rt_hip_plan_set_seeds(plan._h, 1, three) == ERR
    with hip.Plan(pa) as plan:
        lib, h = plan.hl.lib, plan._h
        recs, info = run_set(plan, [pa.seed, pb.seed], None)
        # rejected calls leave the set as it was
        assert lib.rt_hip_plan_set_seeds(h, 3, two) == ERR
        assert lib.rt_hip_plan_set_seeds(h, -1, two) == ERR
        assert lib.rt_hip_plan_set_seeds(h, 2, None) == ERR
        short = rt.Seed(list(pa.seed.x[:4]) + [pa.seed.x[4][:-1].copy()], list(pa.seed.f[:4]) + [pa.seed.f[4][:-1].copy()], 1.0)
        wrong = (cabi.RtSeed * 2)(cabi.seed_record(pa.seed, keep), cabi.seed_record(short, keep))
        assert lib.rt_hip_plan_set_seeds(h, 2, wrong) == ERR and b"dim[4]" in lib.rt_hip_last_error()
        hole = (cabi.RtSeed * 2)(cabi.seed_record(pa.seed, keep), cabi.seed_record(pb.seed, keep))
        hole[1].f[2] = cabi.c_double_p()
        assert lib.rt_hip_plan_set_seeds(h, 2, hole) == ERR and b"incomplete" in lib.rt_hip_last_error()
        plan.run()
        after = plan.fetch_seed_steps()
        for s, p in enumerate((pa, pb)):
            gate_step(after[s], recs[s], p, counts_from_oracle(oracle, p, None), "reordering", f"after rejected set_seeds / seed {s}")
        # with a set installed
        assert lib.rt_hip_plan_fetch_seed_step(h, 2, None, None, None, None) == ERR
        assert lib.rt_hip_plan_seed_step_ptrs(h, 2, None, None, None) == ERR
        assert lib.rt_hip_plan_fetch_seed_step(h, 0, None, None, None, None) == cabi.RT_OK
        assert lib.rt_hip_plan_enable_spectra(h, 1) == ERR
        assert lib.rt_hip_plan_enable_path(h, 1) == ERR
        dev = torch.device("cuda", 0)
        ang = torch.zeros(b.na * b.nb + 8, dtype=torch.float64, device=dev)
        assert lib.rt_hip_plan_run(h, None, None, C.c_void_p(ang.data_ptr())) == ERR
        lent = torch.zeros(b.nv + b.nx * b.ny + 64, dtype=torch.float64, device=dev)
        plan.set_step_buffers(lent.data_ptr(), lent.data_ptr() + 8 * b.nv)
        assert lib.rt_hip_plan_run(h, None, None, None) == ERR and b"lent" in lib.rt_hip_last_error()
        plan.set_step_buffers(0, 0)
        plan.enable_step(False)
        assert lib.rt_hip_plan_run(h, None, None, None) == ERR and b"step mode" in lib.rt_hip_last_error()
        assert lib.rt_hip_plan_enable_spectra(h, 1) == ERR and lib.rt_hip_plan_enable_path(h, 1) == ERR
        plan.enable_step().enable_probe().set_timing_ring(4)
        plan.run()
        probe = plan.fetch_probe()
        final = plan.fetch_seed_steps()
        info = plan.fetch()
        assert int(probe["steps"].sum()) == info["stats"]["cell_steps"]
        march_ms, freq_ms = plan.kernel_times()
        assert march_ms > 0 and freq_ms > 0 and len(plan.ring_times()) == 1
        for s, p in enumerate((pa, pb)):
            gate_step(final[s], recs[s], p, counts_from_oracle(oracle, p, None), "reordering", f"probe and ring on / seed {s}")
        # the blocks: n_seed equal strides inside one allocation; step_ptrs serves seed 0
        p0, p1 = plan.seed_step_ptrs(0), plan.seed_step_ptrs(1)
        stride = p1[0] - p0[0]
        assert stride > 0 and stride % 256 == 0 and all(y - x == stride for x, y in zip(p0, p1))
        assert p0[0] < p0[1] < p0[2] < p1[0] and p0[1] - p0[0] >= 8 * b.nv and p0[2] - p0[1] >= 8 * b.nx * b.ny
        assert stride - (p0[2] - p0[0]) >= 8 * b.na * b.nb
        assert plan.step_ptrs() == p0[:2]
        views = plan.seed_step_tensors()
        torch.cuda.synchronize()
        for s in range(2):
            assert views[s]["E_v"].shape == (b.nv,) and views[s]["nf"].shape == (b.ny, b.nx) and views[s]["I_ang"].shape == (b.nb, b.na)
            for key in ("E_v", "nf", "I_ang"):
                assert np.array_equal(views[s][key].cpu().numpy().reshape(-1), final[s][key]), (s, key)
    out = hip.seed_step_loop(pa, [pa.seed, pb.seed])
    assert out["failure_code"] == 0 and len(out["records"]) == 2 and out["stats"]["n_rays"] == 450
    for s, p in enumerate((pa, pb)):
        gate_step(out["records"][s], recs[s], p, counts_from_oracle(oracle, p, None), "reordering", f"seed_step_loop / seed {s}")
