"""The loop shell of the march (raytrace-miniapp_amd/csrc/rt_march.hip, march_wave): the loop's one exit at its latch, the
count of live lanes n_live that the loop head hands to the blocks, and "does block [A] run" as one comparison of counts,
n_want >= min(park_at, n_live), behind a scalar branch.  None of it may change what a ray's march writes -- parking decides
WHEN a lane's cell set-up runs, never what it computes -- so every case compares the march records (uint32 views of gvl and
evl, ivl and the step counts, the escape flag) and the four launch counters with the oracle's probe, bit for bit, in the
one-launch run and in the two kernels.

What can go wrong is a matter of how many lanes hold a ray, so the launches are small: ray grids of 1, 63, 64, 65 and 193
rays of ASE_small's tables (2 x 1 pixels, tests/test_gpu_retire_batch.py) -- waves with few live lanes, where the threshold
is the adaptive fifth and where n_live < P.park decides; RT_HIP_MARCH_PARK = 1, 12 and 64 on the 65- and 193-ray grids, each
value in a child process of its own; every case on the backward method (the shipped pair, instance MODE 1) and on the
forward one (MODE 0, the switches read at run time); the unbounded instance (RT_HIP_MARCH_IEEE=1, which carries the
watchdog in the loop head) on the 65-ray grid.

The oracle marches the first 193 rays of either method once; a smaller launch is a prefix of it."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import method_pairs as mp
from conftest import GOLDEN, ROOT, rel_l2

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 193]
PARKED_SIZES = [65, 193]
N_REF = max(SIZES)
METHODS = ["backward", "forward"]
_cache = {}


def problem(ase_small, method):
    if method not in _cache:
        base = problem_mod.regrid_beam(ase_small, nx=2, ny=1)
        assert base.n_rays_total == 532 and base.method == 1
        _cache[method] = base if method == "backward" else mp.with_method(base, 2)
    return _cache[method]


def reference(oracle, ase_small, method):
    """the oracle's probe of the first N_REF rays of the grid, once per method, left unchanged"""
    key = ("probe", method)
    if key not in _cache:
        p = problem(ase_small, method)
        pr = oracle.probe(p, p.build_rays(np.arange(N_REF, dtype=np.int64)), want_Iv=False)
        assert (pr["err"] == 0).all() and len(pr["steps"]) == N_REF
        for a in pr.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = pr
    return _cache[key]


def expected_counters(pr, n):
    """n_rays, cell_steps, n_escaped, n_skipped of the first n rays, from the probe (n_skipped as tests/test_gpu_retire_batch.py)"""
    skipped = ~pr["gvl"][:n].any(axis=1) & ~pr["evl"][:n].any(axis=1)
    return [n, int(pr["steps"][:n].astype(np.int64).sum()), int((pr["flags"][:n] & 1).sum()), int(skipped.sum())]


def same_records(got, pr, n, label):
    for key in ("gvl", "evl"):
        assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint32), np.ascontiguousarray(pr[key][:n]).view(np.uint32)), (label, key)
    assert np.array_equal(got["ivl"], pr["ivl"][:n]), (label, "ivl")
    assert np.array_equal(got["steps"], pr["steps"][:n]), (label, "steps")
    assert np.array_equal(got["flags"] & 3, pr["flags"][:n] & 3), (label, "flags")


def counters_of(out):
    st = out["stats"]
    return [int(st[k]) for k in ("n_rays", "cell_steps", "n_escaped", "n_skipped")]


def run(hip, p, n, launch):
    """one launch ("one": RT_HIP_FUSED=1) or the two kernels with the probe ("two"): (outputs, march records or None)"""
    os.environ["RT_HIP_FUSED"] = "1" if launch == "one" else "2"
    try:
        with hip.Plan(p) as plan:
            plan.set_ray_grid(count=n)
            if launch == "two":
                plan.enable_probe()
            out = plan.run().fetch()
            out["fused"] = plan.last_fused()
            return out, (plan.fetch_probe() if launch == "two" else None)
    finally:
        os.environ.pop("RT_HIP_FUSED", None)


def check_launch_pair(hip, p, pr, n, label, expect_one_launch):
    want = expected_counters(pr, n)
    two, rec = run(hip, p, n, "two")
    one, _ = run(hip, p, n, "one")
    print(f"{label}: counters two kernels {counters_of(two)} one launch {counters_of(one)} (fused {one['fused']}) oracle {want}")
    assert not two["fused"], label
    if expect_one_launch:
        assert one["fused"], label
    assert counters_of(two) == want and two["failure_code"] == 0, label
    same_records(rec, pr, n, label)
    assert counters_of(one) == want and one["failure_code"] == 0, label
    # (the two runs differ in the order of the atomic deposits alone: 1e-13, as tests/test_gpu_fused.py)
    assert rel_l2(one["image"], two["image"]) < 1e-13 and rel_l2(one["I_ang"], two["I_ang"]) < 1e-13, label


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", SIZES)
def test_small_launches_march_as_the_oracle(hip, oracle, ase_small, n, method):
    p, pr = problem(ase_small, method), reference(oracle, ase_small, method)
    check_launch_pair(hip, p, pr, n, f"{n} rays, {method}", expect_one_launch=method == "backward")


@pytest.mark.parametrize("method", METHODS)
def test_the_unbounded_instance_on_65_rays(hip, oracle, ase_small, method, monkeypatch):
    """BOUNDED = false: the instance with the watchdog counter in the loop head (it never fires here)"""
    monkeypatch.setenv("RT_HIP_MARCH_IEEE", "1")
    p, pr = problem(ase_small, method), reference(oracle, ase_small, method)
    check_launch_pair(hip, p, pr, 65, f"65 rays, {method}, unbounded instance", expect_one_launch=method == "backward")


_CHILD = r"""
import importlib, os, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
rt = importlib.import_module("raytrace-miniapp_amd")
hip = importlib.import_module("raytrace-miniapp_amd.backend")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
import method_pairs as mp
base = problem_mod.regrid_beam(rt.datfile.load({dat!r}), nx=2, ny=1)
out = {{}}
for method, p in (("backward", base), ("forward", mp.with_method(base, 2))):
    for n in {sizes!r}:
        for launch in ("one", "two"):
            os.environ["RT_HIP_FUSED"] = "1" if launch == "one" else "2"
            with hip.Plan(p) as plan:
                plan.set_ray_grid(count=n)
                if launch == "two":
                    plan.enable_probe()
                r = plan.run().fetch()
                st = r["stats"]
                key = f"{{method}}_{{n}}_{{launch}}_"
                out[key + "counters"] = np.array([st["n_rays"], st["cell_steps"], st["n_escaped"], st["n_skipped"]], np.int64)
                out[key + "code"] = np.array([r["failure_code"], int(plan.last_fused())], np.int64)
                out[key + "image"], out[key + "I_ang"] = r["image"], r["I_ang"]
                if launch == "two":
                    pr = plan.fetch_probe()
                    for k in ("gvl", "evl", "ivl", "steps", "flags"):
                        out[key + k] = pr[k]
np.savez({npz!r}, **out)
print("DONE", flush=True)
"""


@pytest.mark.parametrize("park", [1, 12, 64])
def test_parking_thresholds_in_a_process_of_their_own(oracle, ase_small, park, tmp_path):
    """RT_HIP_MARCH_PARK = 1 ([A] runs whenever a lane wants it), 12 (the default) and 64 (above every n_live: the adaptive
    fifth from the first iteration on, and n_live itself where fewer lanes hold a ray), both methods, both launch forms."""
    npz = tmp_path / "park.npz"
    env = dict(os.environ)
    env["RT_HIP_MARCH_PARK"] = str(park)
    env.pop("RT_HIP_FUSED", None)
    code = _CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), dat=str(GOLDEN / "ASE_small.dat.xz"), sizes=PARKED_SIZES, npz=str(npz))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stderr[-2000:]
    got = np.load(npz)
    for method in METHODS:
        pr = reference(oracle, ase_small, method)
        for n in PARKED_SIZES:
            label = f"park {park}, {n} rays, {method}"
            want = expected_counters(pr, n)
            one, two = f"{method}_{n}_one_", f"{method}_{n}_two_"
            print(f"{label}: counters two kernels {got[two + 'counters'].tolist()} one launch {got[one + 'counters'].tolist()} oracle {want}")
            assert got[two + "counters"].tolist() == want and got[two + "code"].tolist() == [0, 0], label
            same_records({k: got[two + k] for k in ("gvl", "evl", "ivl", "steps", "flags")}, pr, n, label)
            assert got[one + "counters"].tolist() == want and got[one + "code"][0] == 0, label
            if method == "backward":
                assert got[one + "code"][1] == 1, label   # the one launch was taken
            assert rel_l2(got[one + "image"], got[two + "image"]) < 1e-13 and rel_l2(got[one + "I_ang"], got[two + "I_ang"]) < 1e-13, label
