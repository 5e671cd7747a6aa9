"""The lane state of the march (raytrace-miniapp_amd/csrc/rt_march.hip) where it decides what a lane does next: whether the
lane's ray has escaped -- one of the lane's states, ST_ESC / ST_DONE_ESC -- and whether the y axis of its length is mirrored
-- a word of the length's header, tested by blocks [A2], [B] and the close of [C].  Both can go wrong per lane, not per
size: 256 rays (tests/march_flags_inputs.py) of which a good share leaves the plasma part-way, a good share completes and a
quarter escapes in its first cell, on both methods, N = 2 and 3, mirrored and two-sided tables, tables in LDS and read in
place, the bounded and the IEEE / unbounded instance, two kernels and one launch.

Two kernels: every ray's march record through the probe -- the uint32 views of gvl, evl and ivl per slot, the exit ray, the
flags (escaped, error -1: the bits the oracle's probe has) and the steps -- equals the oracle's probe.  One launch: the
probe keeps the two kernels (rt_run_shape.h: nothing may want the march records to itself), so the launch is checked by its
counters against the same probe -- ray-steps, escaped rays, failure code -- and by image and I_ang against the two-kernel run
of the same problem, which differ from it in the order of the atomic deposits alone (1e-13, as tests/test_gpu_fused.py)."""
import functools
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_l2
import march_flags_inputs as mf

rt = importlib.import_module("raytrace-miniapp_amd")
pytestmark = pytest.mark.gpu

CASES = [(table, mirrored, N, tab, ieee, launch)
         for table in ("ASE_small", "seed_small") for mirrored in (True, False) for N in (2, 3)
         for tab, launch in (("lds", "two"), ("global", "two"), ("lds", "one")) for ieee in (False, True)]


@functools.lru_cache(maxsize=None)
def problem(table, mirrored, N):
    return mf.flag_problem(rt.datfile.load(GOLDEN / f"{table}.dat.xz"), mirrored, N)


@functools.lru_cache(maxsize=None)
def reference(table, mirrored, N):
    """the oracle's probe of the 256 rays, computed once per problem and left unchanged"""
    from oracle.binding import Oracle, build
    build(ref=False)
    p = problem(table, mirrored, N)
    ora = Oracle().probe(p, p.build_rays(), want_Iv=False)
    for a in ora.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ora


class environment:
    """the switches of rt_run_shape.h for the duration of a run (tests/test_gpu_edges.py, tests/test_gpu_fused.py)"""

    def __init__(self, tab, ieee, launch):
        self.env = {"RT_HIP_FUSED": "1" if launch == "one" else "2"}
        if launch == "one":
            self.env["RT_HIP_FUSED_SEED"] = "1"   # (the gain-only mode takes the one launch only when asked)
        if tab == "global":
            self.env["RT_HIP_MARCH"] = "global"
        if ieee:
            self.env["RT_HIP_MARCH_IEEE"] = "1"

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)


def same_records(pr, ora):
    for key in ("gvl", "evl", "ivl"):
        assert np.array_equal(pr[key].view(np.uint32), ora[key].view(np.uint32)), key
    ok = ora["err"] == 0   # (the reference leaves the exit ray untouched on an error)
    for key in ("x", "y", "a", "b"):
        assert np.array_equal(pr["ray2"][key][ok].view(np.uint32), ora["ray2"][key][ok].view(np.uint32)), f"exit ray {key}"
    assert np.array_equal(pr["flags"] & 3, ora["flags"] & 3)
    assert np.array_equal(pr["steps"], ora["steps"])


@pytest.mark.parametrize("table,mirrored,N", [(t, m, n) for t in ("ASE_small", "seed_small") for m in (True, False) for n in (2, 3)])
def test_the_chosen_rays_hold_every_population(table, mirrored, N):
    """(on the CPU: a change of the fixtures or of the grids must not empty a population)"""
    ora = reference(table, mirrored, N)
    part_way, complete, first_cell = mf.populations(ora, (N - 1) * 3)
    n = len(ora["steps"])
    assert n == 256
    assert part_way.sum() * 10 >= n and complete.sum() * 10 >= n and first_cell.sum() >= 1
    # pixel rows on both sides of y = 0: the mirrored table takes |y| and flips the sign of the y gradient for half the rays
    rays = problem(table, mirrored, N).build_rays()
    assert (rays["y"] < 0).sum() == n // 2 and (rays["y"] > 0).sum() == n // 2


@pytest.mark.parametrize("table,mirrored,N,tab,ieee,launch", CASES)
def test_march_records_of_escaping_and_completing_rays(hip, table, mirrored, N, tab, ieee, launch):
    p, ora = problem(table, mirrored, N), reference(table, mirrored, N)
    part_way, complete, first_cell = mf.populations(ora, (N - 1) * 3)
    assert part_way.sum() * 10 >= 256 and complete.sum() * 10 >= 256 and first_cell.sum() >= 1
    with environment(tab, ieee, launch):
        with hip.Plan(p) as plan:
            plan.set_ray_grid()
            if launch == "two":
                plan.enable_probe()
            out = plan.run().fetch()
            fused = plan.last_fused()
            pr = plan.fetch_probe() if launch == "two" else None
    st = out["stats"]
    assert st["n_rays"] == 256
    assert st["cell_steps"] == int(ora["steps"].astype(np.int64).sum())
    assert st["n_escaped"] == int((ora["flags"] & 1).sum())
    assert out["failure_code"] == (2 if ((ora["flags"] & 2) != 0).any() else 0)
    if launch == "two":
        assert not fused
        same_records(pr, ora)
        return
    if table == "ASE_small" and (mirrored or N == 2):
        # (emission mode on the beam's own ray grid, 64 rays per pixel, tables in LDS; two lengths of the two-sided tables,
        # twice the size, leave no room for the frequency pass beside them: that run keeps the two kernels)
        assert fused
    with environment(tab, ieee, "two"):
        with hip.Plan(p) as plan:
            two = plan.set_ray_grid().run().fetch()
            assert not plan.last_fused()
    assert rel_l2(out["image"], two["image"]) < 1e-13 and rel_l2(out["I_ang"], two["I_ang"]) < 1e-13
    for key in ("n_rays", "cell_steps", "n_escaped", "n_skipped"):
        assert st[key] == two["stats"][key], key


@pytest.mark.parametrize("tab", ["lds", "global"])
@pytest.mark.parametrize("ieee", [False, True])
def test_a_nan_position_and_an_infinite_angle_are_error_minus_one_and_not_marched(hip, tab, ieee):
    """The rule march_wave documents at the refill: a ray whose start holds a NaN (a NaN position inside the box; an
    infinite launch angle, whose tangent is NaN) is given up before its first cell -- escaped, direction zeroed: one empty
    slot, no step, error -1 from the frequency pass -- and the rays beside it march as if it were not there."""
    p, ora = problem("ASE_small", True, 3), reference("ASE_small", True, 3)
    rays = p.build_rays()
    wild = rays[:2].copy()
    wild["x"], wild["y"], wild["a"], wild["b"] = [np.nan, 0.0030], [0.0011, -0.0011], [1.0, np.inf], [0.0, 1.0]
    both = np.concatenate([rays[:100], wild, rays[100:]])
    with environment(tab, ieee, "two"):
        with hip.Plan(p) as plan:
            out = plan.set_rays(both).enable_probe().run().fetch()
            pr = plan.fetch_probe()
    at = np.array([100, 101])
    clean = np.ones(len(both), bool)
    clean[at] = False
    assert out["failure_code"] == 1 << 1                      # error -1
    assert np.array_equal(pr["flags"][at] & 2, [2, 2])
    assert np.array_equal(pr["steps"][at], [0, 0])
    for key in ("gvl", "evl", "ivl"):
        assert not pr[key][at].view(np.uint32).any(), key     # nothing marched: every slot reads as zero
    assert out["stats"]["cell_steps"] == int(ora["steps"].astype(np.int64).sum())
    same_records({k: v[clean] for k, v in pr.items()}, ora)
