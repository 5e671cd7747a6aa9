"""The step record from all devices of a node (rt_hip_multi_step_loop) and E_v / nf in the caller's memory
(rt_hip_plan_set_step_buffers).

The GPU box has ONE device: n_devices = 1 runs the real (degenerate) RCCL communicator, RT_HIP_MULTI_LOOPBACK = n rehearses
n workers on device 0 with the collective replaced by copies into the receive layout and the sum kernel -- partition,
buffers and assembly of the N > 1 path without the RCCL calls themselves, which are unmeasured on hardware here.

Gates (tests/element_gate.py through gate_step of tests/test_gpu_step.py, every element): against rt_hip_step_loop of the
same rays "reordering" -- (n_e + K) 2^-52, an element nothing deposits into exactly 0 --, against the reduced cubes of the
reference fixture and of the oracle DEFAULT_TIER, in seeded mode TIGHT_TIER.  The figures are printed before every
assertion.  References are computed once per session and shared (the dictionaries below); nobody writes into them."""
import ctypes as C
import importlib

import numpy as np
import pytest

from element_gate import DEFAULT_TIER, TIGHT_TIER, contribution_counts, counts_from_oracle
from test_gpu_step import _ray_set, failing_inputs, gate_step, reduced, same_step_outputs_in_a_failing_run

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu

_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def case(name, ase_small, seed_small):
    """(problem, ray list, tier against the oracle) of the named case; lists and problems are built once."""
    def make():
        if name == "grid_3x2x5x7":      # 210 rays: at 8 workers 27 or 26 each, one ragged tile per device, pixel runs cut by the stride
            p = problem_mod.regrid_beam(ase_small, nx=3, ny=2, na=5, nb=7)
            assert p.n_rays_total == 210
            return p, p.build_rays(), DEFAULT_TIER
        if name == "ase_0.3":
            p = rt.scale_problem(ase_small, 0.3)
            return p, p.build_rays(), DEFAULT_TIER
        if name == "seed_0.02":
            p = rt.scale_problem(seed_small, 0.02)
            return p, p.build_rays(), TIGHT_TIER
        if name == "list_7_-3_5":
            return ase_small, ase_small.build_rays()[7:-3:5].copy(), DEFAULT_TIER
        if name == "grid_1x1x2x3":      # 6 rays
            p = problem_mod.regrid_beam(ase_small, nx=1, ny=1, na=2, nb=3)
            assert p.n_rays_total == 6
            return p, p.build_rays(), DEFAULT_TIER
        raise KeyError(name)
    return once(("case", name), make)


def counts_of(oracle, p, rays, whole_grid):
    if p.seed is not None:
        return counts_from_oracle(oracle, p, None if whole_grid else rays)
    return contribution_counts(p, None if whole_grid else rays)


# ---------------------------------------------------------------------------------------------- 1 - 3: one device, RCCL
def test_one_device_real_communicator(hip, ase_small, ase_ref):
    p = ase_small
    rays = once("ase_rays", p.build_rays)
    out = hip.multi_step_loop(p, rays, n_devices=1)
    assert out["mode"] == 3 and out["failure_code"] == 0 and len(out["failed_rays"]) == 0
    assert out["stats"]["cell_steps"] == 4768067 and out["stats"]["n_rays"] == 399000
    one = once("ase_step_loop", lambda: hip.step_loop(p, rays))
    counts = contribution_counts(p)
    gate_step(out, one, p, counts, "reordering", "multi step: ASE_small, one device, against rt_hip_step_loop")
    gate_step(out, reduced(hip, p, ase_ref), p, counts, DEFAULT_TIER, "multi step: ASE_small, one device, against the reference fixture")


def test_seeded_one_device(hip, oracle, seed_small):
    p = rt.scale_problem(seed_small, 0.05)
    out = hip.multi_step_loop(p, n_devices=1)
    ref = oracle.image_loop(p, n_threads=8)
    assert out["mode"] == 3 and out["failure_code"] == ref["failure_code"] == 0
    assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"] and out["stats"]["n_rays"] == p.n_rays_total
    gate_step(out, reduced(hip, p, ref), p, counts_from_oracle(oracle, p), TIGHT_TIER, "multi step: seeded, one device, against the oracle")


def test_a_list_that_is_no_grid_is_chunked(hip, oracle, ase_small):
    rays = ase_small.build_rays()[5:-11:3].copy()
    out = hip.multi_step_loop(ase_small, rays, n_devices=1)
    ref = oracle.image_loop(ase_small, rays, n_threads=8)
    assert out["mode"] == 2 and out["failure_code"] == 0
    assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"] and out["stats"]["n_rays"] == len(rays)
    gate_step(out, reduced(hip, ase_small, ref), ase_small, contribution_counts(ase_small, rays), DEFAULT_TIER,
              "multi step: arbitrary list as chunks, one device, against the oracle")


def test_a_list_that_only_looks_like_a_grid_ends_the_speculative_attempt(hip, oracle, ase_small, monkeypatch):
    """One ray moved: the periods still say "grid", the devices start on the strided grid, the ray-by-ray check says no
    before anything travels, the second attempt traces chunks of the list itself."""
    odd = once("ase_rays", ase_small.build_rays).copy()
    odd["x"][123457] = odd["x"][0]
    assert hip.ray_list_grid_dims(odd) is None
    ref = oracle.image_loop(ase_small, odd, n_threads=8)
    want = reduced(hip, ase_small, ref)
    counts = contribution_counts(ase_small, odd)
    for loop in ("", "3"):
        if loop:
            monkeypatch.setenv("RT_HIP_MULTI_LOOPBACK", loop)
        out = hip.multi_step_loop(ase_small, odd)
        assert out["mode"] == 2 and out["failure_code"] == 0
        assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"] and out["stats"]["n_rays"] == len(odd)
        gate_step(out, want, ase_small, counts, DEFAULT_TIER, f"multi step: look-alike list, loop-back '{loop}', against the oracle")


# ---------------------------------------------------------------------------------------------- 4, 5: several workers
@pytest.mark.parametrize("name", ["grid_3x2x5x7", "ase_0.3", "seed_0.02", "list_7_-3_5"])
@pytest.mark.parametrize("ndev", [2, 3, 5, 8])
def test_loopback_partition_and_sum(hip, oracle, ase_small, seed_small, monkeypatch, ndev, name):
    p, rays, tier = case(name, ase_small, seed_small)
    whole = not name.startswith("list")
    one = once(("step_loop", name), lambda: hip.step_loop(p, rays))     # (before the variable is set: one device, no workers)
    counts = once(("counts", name), lambda: counts_of(oracle, p, rays, whole))
    monkeypatch.setenv("RT_HIP_MULTI_LOOPBACK", str(ndev))
    out = hip.multi_step_loop(p, rays)
    assert out["mode"] == (3 if whole else 2) and out["failure_code"] == one["failure_code"] == 0
    assert out["stats"]["n_rays"] == len(rays) and out["stats"]["cell_steps"] == one["stats"]["cell_steps"]
    gate_step(out, one, p, counts, "reordering", f"multi step: {name}, {ndev} workers (loop-back), against rt_hip_step_loop")
    if name in ("grid_3x2x5x7", "ase_0.3"):
        ref = once(("oracle", name), lambda: reduced(hip, p, oracle.image_loop(p, rays, n_threads=8)))
        gate_step(out, ref, p, counts, DEFAULT_TIER, f"multi step: {name}, {ndev} workers (loop-back), against the oracle")


def test_more_workers_than_rays(hip, oracle, ase_small, seed_small, monkeypatch):
    p, rays, _ = case("grid_1x1x2x3", ase_small, seed_small)
    one = hip.step_loop(p, rays)
    monkeypatch.setenv("RT_HIP_MULTI_LOOPBACK", "8")           # workers 6 and 7 trace nothing and add a record of zeros
    out = hip.multi_step_loop(p, rays)
    assert out["mode"] == 3 and out["failure_code"] == 0
    assert out["stats"]["n_rays"] == 6 and out["stats"]["cell_steps"] == one["stats"]["cell_steps"]
    gate_step(out, one, p, contribution_counts(p, rays), "reordering", "multi step: 6 rays on 8 workers (loop-back), against rt_hip_step_loop")
    assert one["E_v"].any() and one["nf"].any()


# ---------------------------------------------------------------------------------------------- 6: failing runs
@pytest.mark.parametrize("which", ["invalid_ray", "nan_lineshape", "negative_lineshape"])
def test_failing_runs_at_three_workers(hip, oracle, ase_small, which, monkeypatch):
    """Every worker with failing rays runs its checking repeat before its record travels: the sum is the reduction of
    what the CPU loop leaves.  401 (NaN) and 351 (negative) of the 401 rays fail and a report holds RT_N_FAILED_MAX = 32:
    every entry reports the first 32 of them in list order (plan_report_first_failed), so the chunks of the list, taken
    in device order, give the report of rt_hip_step_loop."""
    p, rays, bit = failing_inputs(ase_small)[which]
    one = hip.step_loop(p, rays)
    ora = oracle.image_loop(p, rays)
    monkeypatch.setenv("RT_HIP_MULTI_LOOPBACK", "3")
    out = hip.multi_step_loop(p, rays)
    assert ora["failure_code"] & bit and out["failure_code"] == ora["failure_code"] == one["failure_code"]
    assert out["mode"] == 2 and out["stats"]["n_rays"] == len(rays)
    ref = reduced(hip, p, ora)
    if which == "invalid_ray":
        assert len(out["failed_rays"]) == 1 and out["failed_rays"][0] == rays[7]
        counts = counts_from_oracle(oracle, p, rays)           # (the failing ray is not counted)
        gate_step(out, ref, p, counts, DEFAULT_TIER, "multi step: error -1 at 3 workers against the oracle's cube")
        gate_step(out, one, p, counts, "reordering", "multi step: error -1 at 3 workers against rt_hip_step_loop")
    else:
        same_step_outputs_in_a_failing_run(out, ref)
        same_step_outputs_in_a_failing_run(out, one)
    # what is reported: failing rays only, as many as rt_hip_step_loop reports
    _, err = oracle.exit_rays(p, rays)
    failing = set(_ray_set(rays[err != 0]))
    got, want = _ray_set(out["failed_rays"]), _ray_set(one["failed_rays"])
    print(f"failing run / {which}: {len(failing)} of {len(rays)} rays fail, reported {len(got)} (rt_hip_step_loop {len(want)}), "
          f"in both reports {len(set(got) & set(want))}")
    assert set(got) <= failing and len(got) == len(want) == min(len(failing), rt.cabi.RT_N_FAILED_MAX)
    assert got == want                                         # (as sets: the order is by device)
    assert got == _ray_set(rays[err != 0][:rt.cabi.RT_N_FAILED_MAX])       # the rays the CPU loop pushes first


@pytest.mark.parametrize("first,stride", [(0, 1), (3, 2)])
def test_the_report_of_a_failing_ray_grid_is_the_first_rays_in_list_order(hip, oracle, ase_small, first, stride):
    """The same rule on rays generated on the device (whole and strided grid), in step mode and in image mode."""
    import copy
    neg, _, bit = failing_inputs(ase_small)["negative_lineshape"]
    p = copy.copy(problem_mod.regrid_beam(neg, nx=3, ny=4, na=5, nb=7))
    p.N_start, p.N_parallel = first, stride
    rays = p.build_rays()
    _, err = oracle.exit_rays(p, rays)
    failing = rays[err != 0]
    print(f"failing ray grid, first {first} stride {stride}: {len(failing)} of {len(rays)} rays fail")
    assert len(failing) > rt.cabi.RT_N_FAILED_MAX and set(np.unique(err)) <= {0, -2}
    for step in (True, False):
        with hip.Plan(p) as plan:
            plan.set_ray_grid().enable_step(step).run()
            out = plan.fetch()
        assert out["failure_code"] == bit and out["stats"]["n_rays"] == len(rays)
        assert _ray_set(out["failed_rays"]) == _ray_set(failing[:rt.cabi.RT_N_FAILED_MAX]), step


# ---------------------------------------------------------------------------------------------- 7: borrowed buffers
GUARD, SENTINEL = 64, -12345.0


class Lent:
    """E_v, nf and I_ang as views of ONE tensor, GUARD doubles of SENTINEL before, between and behind them."""

    def __init__(self, p):
        import torch
        b = p.beam
        self.sizes = (b.nv, b.nx * b.ny, b.na * b.nb)
        self.t = torch.full((4 * GUARD + sum(self.sizes),), SENTINEL, dtype=torch.float64, device=torch.device("cuda", 0))
        self.views, at = [], GUARD
        for n in self.sizes:
            self.views.append(self.t[at:at + n])
            at += n + GUARD
        self.E_v, self.nf, self.iang = self.views

    def guards_intact(self):
        import torch
        torch.cuda.synchronize()
        h, at = self.t.cpu().numpy(), 0
        for n in self.sizes + (0,):
            if not (h[at:at + GUARD] == SENTINEL).all():
                return False
            at += GUARD + n
        assert at == len(h)
        return True

    def record(self):
        import torch
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in zip(("E_v", "nf", "I_ang"), self.views)}


@pytest.mark.parametrize("name", ["every_499th", "grid_3x2x5x7"])
def test_borrowed_step_buffers(hip, ase_small, seed_small, name):
    cabi = rt.cabi
    if name == "every_499th":
        p = ase_small
        rays = p.build_rays(np.arange(0, p.n_rays_total, 499, dtype=np.int64))
    else:
        p, rays, _ = case(name, ase_small, seed_small)
    counts = contribution_counts(p, rays)
    buf = Lent(p)
    with hip.Plan(p) as plan:
        lib, h = plan.hl.lib, plan._h
        # accepted outside step mode, takes effect when step mode is switched on
        plan.set_rays(rays).set_step_buffers(buf.E_v.data_ptr(), buf.nf.data_ptr()).enable_step()
        plan.run(iang_ptr=buf.iang.data_ptr())
        lent = plan.fetch_step()
        assert plan.fetch()["failure_code"] == 0
        assert plan.step_ptrs() == (buf.E_v.data_ptr(), buf.nf.data_ptr())
        assert buf.guards_intact()
        in_place = buf.record()
        for key in ("E_v", "nf", "I_ang"):
            assert np.array_equal(in_place[key], lent[key]), key       # fetch_step serves the buffers the run used
        # a second run: zeroed by the run, not accumulated
        plan.run(iang_ptr=buf.iang.data_ptr())
        again = plan.fetch_step()
        assert buf.guards_intact()
        gate_step(again, lent, p, counts, "reordering", f"borrowed buffers, {name}: second run against the first")
        # (0, 0): the plan's own allocation again; the caller's tensor is not touched any more
        buf.t.fill_(SENTINEL)
        plan.set_step_buffers(0, 0).run()
        own = plan.fetch_step()
        e, n = plan.step_ptrs()
        assert e and n and e != buf.E_v.data_ptr() and n != buf.nf.data_ptr()
        assert (buf.t.cpu().numpy() == SENTINEL).all()
        gate_step(lent, own, p, counts, "reordering", f"borrowed buffers, {name}: lent against the plan's own")
        assert own["E_v"].any() and own["nf"].any() and own["I_ang"].any()
        # a misaligned nf pointer, and one pointer without the other
        assert lib.rt_hip_plan_set_step_buffers(h, C.c_void_p(buf.E_v.data_ptr()), C.c_void_p(buf.nf.data_ptr() + 4)) == cabi.RT_ERR_ARG
        assert lib.rt_hip_plan_set_step_buffers(h, C.c_void_p(buf.E_v.data_ptr() + 2), C.c_void_p(buf.nf.data_ptr())) == cabi.RT_ERR_ARG
        assert lib.rt_hip_plan_set_step_buffers(h, C.c_void_p(buf.E_v.data_ptr()), None) == cabi.RT_ERR_ARG
        assert lib.rt_hip_plan_set_step_buffers(h, None, C.c_void_p(buf.nf.data_ptr())) == cabi.RT_ERR_ARG
        # (a refused call changes nothing: still the plan's own)
        plan.run()
        assert plan.step_ptrs() == (e, n) and (buf.t.cpu().numpy() == SENTINEL).all()


def test_the_checking_repeat_writes_the_borrowed_buffers(hip, ase_small):
    """A failing run (error -2) is repeated without its failing rays: the repeat zeroes and fills the caller's buffers."""
    p, rays, bit = failing_inputs(ase_small)["negative_lineshape"]
    buf = Lent(p)
    with hip.Plan(p) as plan:
        plan.set_rays(rays).enable_step().run()
        own = plan.fetch_step()
        code = plan.fetch()["failure_code"]
        plan.set_step_buffers(buf.E_v.data_ptr(), buf.nf.data_ptr()).run(iang_ptr=buf.iang.data_ptr())
        lent = plan.fetch_step()
        assert plan.fetch()["failure_code"] == code and code & bit
    assert buf.guards_intact()
    in_place = buf.record()
    for key in ("E_v", "nf", "I_ang"):
        assert np.array_equal(in_place[key], lent[key]), key
    same_step_outputs_in_a_failing_run(lent, own)


# ---------------------------------------------------------------------------------------------- 8: contract
def test_contract(hip, ase_small, seed_small, monkeypatch):
    cabi = rt.cabi
    lib = hip.HipLibrary.get().lib
    p, rays, _ = case("grid_3x2x5x7", ase_small, seed_small)
    m = cabi.Marshalled(p)
    b = p.beam
    E_v, nf, iang = np.zeros(b.nv), np.zeros(b.nx * b.ny), np.zeros(b.na * b.nb)
    code = C.c_uint(0)

    def call(beam=True, gain=True, e=True, n=True, a=True, have_rays=True):
        return lib.rt_hip_multi_step_loop(1, m.N, C.byref(m.beam) if beam else None, m.gain if gain else None, m.seed_ref, p.method,
                                          cabi.rays_ptr(rays) if have_rays else None, len(rays), p.scale,
                                          cabi._dp(E_v) if e else None, cabi._dp(nf) if n else None, cabi._dp(iang) if a else None,
                                          C.byref(code), None, 0, None, None)

    for missing in ("beam", "gain", "e", "n", "a", "have_rays"):
        assert call(**{missing: False}) == cabi.RT_ERR_ARG, missing
    assert call() == cabi.RT_OK and lib.rt_hip_multi_last_mode() == 3 and code.value == 0
    assert E_v.any() and nf.any() and iang.any()
    # the image arm reports 1 and 2 as before
    q, q_rays, _ = case("ase_0.3", ase_small, seed_small)
    assert hip.multi_image_loop(q, q_rays, n_devices=1)["mode"] == 1
    assert hip.multi_image_loop(q, q_rays[3:-5:2].copy(), n_devices=1)["mode"] == 2
    assert hip.multi_step_loop(q, q_rays[3:-5:2].copy(), n_devices=1)["mode"] == 2
