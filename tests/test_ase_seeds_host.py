"""ASE seeds on an emission plan (rt_hip_plan_set_ase_seeds, rt_step_ase_seeds_kernel), the parts that need no device.

1. The premise, on the CPU oracle: the march of a problem does not depend on use_emis apart from evl -- gvl, ivl, the exit
   ray, flags bits 0-1 and the step count of p and of carry(p, seed) are bit-equal and the seeded evl is all zero.  Both
   methods, N = 3 and 5, plain and dark.
2. The census of the inputs of tests/test_gpu_ase_seeds.py (tests/ase_seeds.py) as conditions, so that the GPU tests cannot
   pass on inputs that stopped exercising what they are there for.
3. rt_hip_debug_run_shape with use_emis, n_seed = 2 and step_on: pass_kind 7, the LDS of the seed-set formula with three
   records, two kernels whatever set_step_one_launch says, global atomics once three histograms exceed the limit.
4. Header and binding carry the four symbols; the Python face has its methods and refuses what it can before any native
   call."""
import ctypes
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import ase_seeds as A

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_set_ase_seeds", "rt_hip_plan_fetch_full_step", "rt_hip_plan_full_step_ptrs", "rt_hip_full_step_loop"]

CASES = [(1, 3, False), (2, 3, False), (1, 5, False), (2, 5, False), (1, 3, True), (2, 3, True), (1, 5, True), (2, 5, True)]

_probes = {}


def probe(oracle, p, rays):
    if id(p) not in _probes:
        _probes[id(p)] = (p, oracle.probe(p, rays, want_Iv=False))
    return _probes[id(p)][1]


# ---------------------------------------------------------------------------------------------- 1. the premise
@pytest.mark.parametrize("method,N,dark", CASES)
def test_the_march_does_not_depend_on_the_emission_switch(oracle, ase_small, method, N, dark):
    p = A.base(ase_small, method, N, dark)
    rays = p.build_rays()
    assert len(rays) == 1440
    mine = probe(oracle, p, rays)
    assert mine["evl"].any()
    for seed in A.seeds_of(p):
        q = A.carry(p, seed)
        other = oracle.probe(q, rays, want_Iv=False)
        for key in ("gvl", "ivl", "steps"):
            assert np.array_equal(mine[key], other[key]), key
        assert mine["gvl"].tobytes() == other["gvl"].tobytes()
        assert mine["ray2"].tobytes() == other["ray2"].tobytes()
        assert np.array_equal(mine["flags"] & 3, other["flags"] & 3)
        assert not other["evl"].any()


# ---------------------------------------------------------------------------------------------- 2. the census
@pytest.mark.parametrize("method,N,dark", CASES)
def test_census_of_the_inputs(oracle, ase_small, method, N, dark):
    p = A.base(ase_small, method, N, dark)
    rays = p.build_rays()
    pr = probe(oracle, p, rays)
    escaped = (pr["flags"] & 1) != 0
    pts = A.seed_points(p, pr, rays)
    assert not (pr["err"] != 0).any()                      # no failure anywhere
    assert 40 <= int(escaped.sum()) < 1440                 # escaped rays: seed factor 0, live for the ASE record
    sets = []
    for seed in A.seeds_of(p):
        inside = A.in_range(seed, pts) & ~escaped
        print(f"method {method}, N = {N}, dark = {dark}: escaped {int(escaped.sum())}, in range {int(inside.sum())}")
        assert int(inside.sum()) >= 40
        sets.append(inside)
        err = np.asarray(oracle.exit_rays(A.carry(p, seed), rays)[1])
        assert not (err != 0).any()
    assert not np.array_equal(sets[0], sets[1])
    if dark:
        zero = ~pr["gvl"].any(axis=1) & ~pr["evl"].any(axis=1)
        print(f"    all sums zero: {int(zero.sum())}, of them in range of `wide`: {int((zero & sets[0]).sum())}")
        # (N = 3: the inputs of the dark test proper; N = 5 sends the generic instance through the same paths on fewer such rays)
        assert int((zero & sets[0]).sum()) >= (300 if N == 3 else 150)
        assert int((~zero).sum()) >= 300
        # whole 64-ray tiles in the dark: no ray of theirs is live for the ASE record, all are for the seed records
        assert sum(bool(zero[t:t + 64].all()) for t in range(0, 1440, 64)) >= 2
    if not dark:
        qn = A.carry(p, A.negative(A.seeds_of(p)[1]))
        err = np.asarray(oracle.exit_rays(qn, rays)[1])
        assert int((err == -2).sum()) >= cabi.RT_N_FAILED_MAX + 1 == 33 and not (err == -1).any() and not (err == -3).any()


# ---------------------------------------------------------------------------------------------- 3. the run shape
CU, LDS = 256, 160 * 1024
EXP_TAB, XP_ROW, WG_WAVES = 256, 66, 16


def shape(**facts):
    hl = backend.HipLibrary.get()
    f = cabi.RtRunFacts(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, blob_bytes=40000, tables_bounded=1,
                        c_h3=0.025, march_prune=1, ntest_proven=1, occupancy_per_cu=1, method=1, step_on=1, n_seed=2,
                        use_emis=1, L=2, n_rays=1 << 20, n_tiles=1 << 14)
    for k, v in facts.items():
        assert hasattr(f, k), k
        setattr(f, k, v)
    out = cabi.RtRunShape(size=ctypes.sizeof(cabi.RtRunShape))
    rc = hl.lib.rt_hip_debug_run_shape(ctypes.byref(f), ctypes.byref(out))
    assert rc == 0, hl.lib.rt_hip_last_error()
    return out


def lds_by_hand(in_lds, n_ang, Kp, n_rec):
    """The seed-set formula: [2 EXP_TAB | n_rec (n_ang + 3 & ~1) | n_rec Kp | 16 x 4 x 66] doubles."""
    return 8 * (2 * EXP_TAB + n_rec * (((n_ang + 3) & ~1 if in_lds else 0) + Kp) + WG_WAVES * 4 * XP_ROW)


@pytest.fixture()
def no_knobs(monkeypatch):
    import os
    for k in list(os.environ):
        if k.startswith("RT_HIP_"):
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("method", [1, 2])
def test_shape_of_two_ase_seeds(no_knobs, method):
    out = shape(K=64, Kp=64, n_iang=20, method=method, own_cells=1 if method == 1 else 0, rays_per_pixel=64, step_one_launch=1)
    assert out.kind == 0                                   # two kernels, whatever set_step_one_launch says
    assert out.pass_kind == 7 and out.pass_in_lds == 1 and out.pass_wg_waves == WG_WAVES and out.pass_grid == CU
    assert out.pass_lds == 8 * (512 + 3 * (22 + 64) + 4224) == lds_by_hand(True, 20, 64, 3) <= LDS
    assert out.key_emis == 1
    one = shape(K=64, Kp=64, n_iang=20, method=method, n_seed=1)
    assert one.pass_kind == 7 and one.pass_lds == lds_by_hand(True, 20, 64, 2)
    # the neighbours of the new kind keep theirs: no seeds, a seeded plan's set, a scan
    assert shape(K=64, Kp=64, n_iang=20, method=method, n_seed=0).pass_kind == 2
    assert shape(K=64, Kp=64, n_iang=20, method=method, use_emis=0).pass_kind == 3
    assert shape(K=64, Kp=64, n_iang=20, method=2, n_seed=0, scan_on=1, L=4).pass_kind == 5


def test_three_histograms_that_do_not_fit_take_global_atomics(no_knobs):
    # one histogram of 4000 cells is 32 KB and stays in LDS; three, with their E_v accumulators, fit; with 1200 frequencies they do not
    out = shape(K=84, Kp=84, n_iang=4000)
    assert out.pass_kind == 7 and out.pass_in_lds == 1 and out.pass_lds == lds_by_hand(True, 4000, 84, 3) <= LDS
    assert lds_by_hand(True, 4090, 1200, 3) > LDS
    out = shape(K=1200, Kp=1200, n_iang=4090)
    assert out.pass_kind == 7 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 4090, 1200, 3) <= LDS
    out = shape(K=84, Kp=84, n_iang=4097)                   # (above 32 KB no step pass keeps the histogram in LDS)
    assert out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 4097, 84, 3)


def test_accumulators_that_do_not_fit_are_reported_as_such(no_knobs):
    out = shape(K=8192, Kp=8192, n_iang=20)
    assert out.pass_kind == 7 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 20, 8192, 3) > LDS


# ---------------------------------------------------------------------------------------------- 4. header, binding, Python face
def test_entry_points_are_declared_listed_and_bound():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(rt_hip_[a-z_0-9]+)\s*\(", text))
    lib = backend.HipLibrary.get().lib
    for name in NEW:
        assert name in cabi.HIP_API_SYMBOLS, name
        assert name in declared, name
        assert getattr(lib, name).restype is ctypes.c_int, name
    assert re.search(r"int\s+rt_hip_plan_set_ase_seeds\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+n_seed,\s*const\s+rt_seed\s*\*\s*seeds,"
                     r"\s*const\s+double\s*\*\s*scales\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_fetch_full_step\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+r,\s*double\s*\*\s*E_v,\s*double\s*\*\s*nf,"
                     r"\s*double\s*\*\s*I_ang,\s*unsigned\s+int\s*\*\s*failure_code\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_full_step_ptrs\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+r,\s*double\s*\*\*\s*E_v_dev,"
                     r"\s*double\s*\*\*\s*nf_dev,\s*double\s*\*\*\s*iang_dev\s*\)", text)
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\s*\((.*?)\)", text, flags=re.S).group(1).split(",")]
    plain, mine = args("rt_hip_step_loop"), args("rt_hip_full_step_loop")
    assert [a for a in mine if a not in ("n_seed", "seeds", "scales")] == [a if a != "failure_code" else "failure_codes" for a in plain if a != "seed"]
    assert len(lib.rt_hip_full_step_loop.argtypes) == len(lib.rt_hip_step_loop.argtypes) + 2
    assert len(lib.rt_hip_plan_set_ase_seeds.argtypes) == 4
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"      # (no new fact: use_emis with n_seed > 0 is the case)
    for method in ("set_ase_seeds", "fetch_full_step", "full_step_ptrs", "full_step_tensors"):
        assert callable(getattr(backend.Plan, method)), method
    assert callable(backend.full_step_loop)


class _NoNativeCalls:
    """Stands where Plan.hl stands: any use of the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"Plan.set_ase_seeds reached the native library ({name}) before it refused its arguments")


def test_python_face_refuses_before_any_native_call(ase_small, seed_small):
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None          # (close() has nothing to destroy)
    p = A.base(ase_small, 1)
    w, n = A.seeds_of(p)
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        plan.set_ase_seeds([w] * (cabi.RT_N_SEED_MAX + 1))
    with pytest.raises(ValueError, match="not a Seed"):
        plan.set_ase_seeds([w, None])
    with pytest.raises(ValueError, match="scales"):
        plan.set_ase_seeds([w, n], scales=[1.0])
    with pytest.raises(AssertionError, match="native library"):    # (what is acceptable does go on to the library)
        plan.set_ase_seeds([w, n], scales=[13.3, 13.3])
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        backend.full_step_loop(p, [])
    with pytest.raises(ValueError, match="not a Seed"):
        backend.full_step_loop(p, [w, 3.0])
    with pytest.raises(ValueError, match="scales"):
        backend.full_step_loop(p, [w], scales=[1.0, 2.0])
    with pytest.raises(ValueError, match="carries a seed"):
        backend.full_step_loop(seed_small, [w])


def test_the_loop_raises_without_a_device_and_runs_with_one(ase_small):
    p = A.base(ase_small, 1)
    seeds = list(A.seeds_of(p))
    if backend.HipLibrary.get().device_count() > 0:      # (the parity of these records: tests/test_gpu_ase_seeds.py)
        out = backend.full_step_loop(p, seeds)
        assert out["failure_code"] == 0 and out["stats"]["n_rays"] == 1440 and len(out["seeds"]) == 2
        assert all(rec["E_v"].any() and rec["nf"].any() and rec["I_ang"].any() for rec in [out["ase"]] + out["seeds"])
        return
    with pytest.raises(backend.RayTraceError):
        backend.full_step_loop(p, seeds)
