"""ASE seeds of a length scan (rt_hip_plan_set_scan_ase_seeds, rt_step_scan_ase_seeds_kernel), the parts that need no device.

1. The census of the inputs of tests/test_gpu_scan_ase_seeds.py (tests/scan_ase_seeds.py) on the CPU oracle, as conditions, so
   that the GPU tests cannot pass on inputs that stopped exercising what they are there for.
2. The failure matrix of the failing input, per record and length.
3. rt_hip_debug_run_shape with use_emis, scan_on, n_seed = 2 and step_on: pass kind 8, the scan march unchanged, the LDS of
   the seed-set formula with (1 + n_seed) L records.
4. Header, export map and binding carry the four symbols; the Python face refuses what it can before any native call."""
import ctypes
import fnmatch
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import ase_seeds as A
import length_scan as ls
import scan_ase_seeds as X
from test_seed_scan_host import lds_by_hand

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_set_scan_ase_seeds", "rt_hip_plan_fetch_full_length_step", "rt_hip_plan_full_length_step_ptrs",
       "rt_hip_full_length_scan_loop"]


# ---------------------------------------------------------------------------------------------- 1. the census
def test_census_six_lengths(oracle, ase_small):
    p = A.base(ase_small, 2, 6)
    rays = p.build_rays()
    assert len(rays) == 1440 and len(rays) % 64 == 32 and p.beam.nv == 52
    esc = {n: e for n, (e, _) in ls.escape_census(oracle, p, rays).items()}
    counts = [int(esc[n].sum()) for n in range(2, 7)]
    print(f"N = 6: escaped by n = 2 .. 6: {counts}")
    assert counts == [24, 51, 89, 152, 188]
    assert counts[0] >= 20 and all(b - a >= 20 for a, b in zip(counts, counts[1:]))      # newly escaped rays at every length
    for n in range(3, 7):
        assert not (esc[n - 1] & ~esc[n]).any()                                         # (escaped stays escaped)
    w, nr = A.seeds_of(p)
    in_w = [int((A.in_range(w, rays) & ~esc[n]).sum()) for n in range(2, 7)]
    in_n = [int((A.in_range(nr, rays) & ~esc[n]).sum()) for n in range(2, 7)]
    print(f"N = 6: in range of `wide` and not escaped {in_w}, of `narrow` {in_n}")
    assert in_w[0] == 1416 and in_w[-1] == 1252 and all(a > b for a, b in zip(in_w, in_w[1:]))   # carries its factor below e, 0 from e on
    assert in_n == [48] * 5 and min(in_n) >= 40
    for row in X.problems(p, (w, nr)):
        for n, q in row.items():
            assert oracle.image_loop(q, rays)["failure_code"] == 0, (q.label, n)                 # no failure in any record


def test_census_dark_variant(oracle, ase_small):
    p = A.base(ase_small, 2, 6, dark=True)
    rays = p.build_rays()
    pr = oracle.probe(p, rays, want_Iv=False)
    S = pr["gvl"].shape[1]
    assert S == 15
    zero_all = ~pr["gvl"].any(axis=1) & ~pr["evl"].any(axis=1)
    print(f"dark, N = 6: all sums zero over the whole run: {int(zero_all.sum())}")
    assert int(zero_all.sum()) == 337 >= 300
    extra = {}
    for n in range(2, 6):
        zero_n = ~pr["gvl"][:, :3 * (n - 1)].any(axis=1) & ~pr["evl"][:, :3 * (n - 1)].any(axis=1)
        extra[n] = int((zero_n & ~zero_all).sum())
    print(f"dark, N = 6: zero sums in the prefix only, n = 2 .. 5: {extra}")
    assert extra[2] == 119 and max(extra.values()) >= 20        # not marked: they stay live for the ASE records
    # whole dark tiles: none in grid order at this N, five with the marked rays first (X.dark_first: the list of the GPU test)
    order = X.dark_first(zero_all)
    tiles = [sum(bool(z[t:t + 64].all()) for t in range(0, 1440, 64)) for z in (zero_all, zero_all[order])]
    print(f"dark, N = 6: whole dark tiles in grid order {tiles[0]}, with the marked rays first {tiles[1]}")
    assert tiles[1] == 337 // 64 == 5 and sorted(order.tolist()) == list(range(1440))
    w, _ = A.seeds_of(p)
    assert int((zero_all & A.in_range(w, rays)).sum()) >= 150   # the marked rays carry a seed factor


def test_census_ten_lengths(oracle, ase_small):
    p = A.base(ase_small, 2, 10)
    rays = p.build_rays()
    pr = oracle.probe(p, rays, want_Iv=False)
    assert p.N == 10 and int(((pr["flags"] & 1) != 0).sum()) == 609


# ---------------------------------------------------------------------------------------------- 2. the failure matrix
def test_failure_matrix(oracle, ase_small):
    p = A.base(ase_small, 2, 6)
    f, seeds = X.failing(p)
    rays = f.build_rays()
    rows = X.problems(f, seeds)
    got = [[oracle.image_loop(row[n], rays)["failure_code"] for n in range(2, 7)] for row in rows]
    print(f"failure matrix: {got}")
    assert got == X.WANT_CODES
    m2, m3 = [], []
    for n in range(2, 7):
        err = np.asarray(oracle.exit_rays(rows[2][n], rays)[1])
        assert not (err == -1).any()
        m2.append(int((err == -2).sum()))
        m3.append(int((err == -3).sum()))
    print(f"negated `narrow`: error -2 at n = 2 .. 6 {m2}, error -3 {m3}")
    assert m2 == [48] * 5 and m3 == [0, 0, 84, 84, 84]
    assert m2[0] > cabi.RT_N_FAILED_MAX


# ---------------------------------------------------------------------------------------------- 3. the run shape
CU, LDS = 256, 160 * 1024
WG_WAVES = 16


def shape(**facts):
    hl = backend.HipLibrary.get()
    f = cabi.RtRunFacts(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, blob_bytes=40000, tables_bounded=1,
                        c_h3=0.025, march_prune=1, ntest_proven=1, occupancy_per_cu=1, method=2, step_on=1, scan_on=1, n_seed=2,
                        use_emis=1, L=5, n_rays=1 << 20, n_tiles=1 << 14)
    for k, v in facts.items():
        assert hasattr(f, k), k
        setattr(f, k, v)
    out = cabi.RtRunShape(size=ctypes.sizeof(cabi.RtRunShape))
    rc = hl.lib.rt_hip_debug_run_shape(ctypes.byref(f), ctypes.byref(out))
    assert rc == 0, hl.lib.rt_hip_last_error()
    return out


@pytest.fixture()
def no_knobs(monkeypatch):
    import os
    for k in list(os.environ):
        if k.startswith("RT_HIP_"):
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("one_launch", [0, 1])
def test_shape_of_two_scan_ase_seeds(no_knobs, one_launch):
    L = 5
    out = shape(K=52, Kp=52, n_iang=20, step_one_launch=one_launch)
    assert out.kind == 0                                   # two kernels, whatever set_step_one_launch says
    assert out.pass_kind == 8 and out.pass_in_lds == 1 and out.pass_wg_waves == WG_WAVES and out.pass_grid == CU
    assert out.pass_lds == lds_by_hand(True, 20, 52, 3 * L) == 8 * (512 + 15 * (22 + 52) + 4224) <= LDS
    assert out.key_emis == 1
    # the march is the scan march unchanged
    assert out.mode == 3 and out.opt == 8 and out.last_march_inst == (1 | (8 << 1))
    plain = shape(K=52, Kp=52, n_iang=20, n_seed=0)
    for key in ("mode", "opt", "bounded", "bthr", "grid", "chunk", "mlds", "late_chunks", "last_march_inst"):
        assert getattr(out, key) == getattr(plain, key), key
    one = shape(K=52, Kp=52, n_iang=20, n_seed=1)
    assert one.pass_kind == 8 and one.pass_lds == lds_by_hand(True, 20, 52, 2 * L)
    # the neighbours keep their kinds
    assert plain.pass_kind == 5
    assert shape(K=52, Kp=52, n_iang=20, use_emis=0).pass_kind == 6
    assert shape(K=52, Kp=52, n_iang=20, scan_on=0).pass_kind == 7
    assert shape(K=52, Kp=52, n_iang=20, scan_on=0, use_emis=0).pass_kind == 3
    assert shape(K=52, Kp=52, n_iang=20, scan_on=0, n_seed=0).pass_kind == 2
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"      # (no new fact)


def test_histograms_that_do_not_fit_take_global_atomics(no_knobs):
    L = 5
    assert lds_by_hand(True, 900, 84, 3 * L) <= LDS < lds_by_hand(True, 1500, 84, 3 * L)
    assert shape(K=84, Kp=84, n_iang=900).pass_in_lds == 1
    out = shape(K=84, Kp=84, n_iang=1500)
    assert out.pass_kind == 8 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 1500, 84, 3 * L) <= LDS
    assert shape(K=84, Kp=84, n_iang=1500, n_seed=0).pass_in_lds == 1      # (the plain scan of these numbers keeps them)


def test_accumulators_that_do_not_fit_report_more_than_the_limit(no_knobs):
    out = shape(K=1024, Kp=1024, n_iang=20, L=8)
    assert out.pass_kind == 8 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 20, 1024, 24) > LDS
    assert shape(K=1024, Kp=1024, n_iang=20, L=8, n_seed=0).pass_lds <= LDS


def test_the_serial_mode_is_one_wave(no_knobs, monkeypatch):
    monkeypatch.setenv("RT_HIP_STEP_SERIAL", "1")
    out = shape(K=52, Kp=52, n_iang=20)
    assert out.pass_kind == 8 and out.pass_wg_waves == 1 and out.pass_grid == 1 and out.pass_in_lds == 1
    assert out.pass_lds == 8 * (512 + 15 * (22 + 52) + 1 * 4 * 66)
    assert out.mode == 3 and out.kind == 0


# ---------------------------------------------------------------------------------------------- 4. header, map, binding, Python face
def test_entry_points_are_declared_listed_and_exported():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(rt_hip_[a-z_0-9]+)\s*\(", text))
    lib = backend.HipLibrary.get().lib
    the_map = (ROOT / "raytrace-miniapp_amd" / "csrc" / "rt_hip.map").read_text()
    exported = re.findall(r"global:\s*(.*?)local:", the_map, flags=re.S)[0].replace(";", " ").split()
    for name in NEW:
        assert name in cabi.HIP_API_SYMBOLS, name
        assert name in declared, name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
        assert getattr(lib, name).restype is ctypes.c_int, name
    assert re.search(r"int\s+rt_hip_plan_set_scan_ase_seeds\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+n_seed,\s*const\s+rt_seed\s*\*\s*seeds,"
                     r"\s*const\s+double\s*\*\s*scales\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_fetch_full_length_step\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+r,\s*int\s+n,\s*double\s*\*\s*E_v,"
                     r"\s*double\s*\*\s*nf,\s*double\s*\*\s*I_ang,\s*unsigned\s+int\s*\*\s*failure_code\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_full_length_step_ptrs\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+r,\s*int\s+n,\s*double\s*\*\*\s*E_v_dev,"
                     r"\s*double\s*\*\*\s*nf_dev,\s*double\s*\*\*\s*iang_dev\s*\)", text)
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\s*\((.*?)\)", text, flags=re.S).group(1).split(",")]
    assert args("rt_hip_full_length_scan_loop") == args("rt_hip_full_step_loop")
    assert list(lib.rt_hip_full_length_scan_loop.argtypes) == list(lib.rt_hip_full_step_loop.argtypes)
    assert len(lib.rt_hip_plan_set_scan_ase_seeds.argtypes) == 4 and len(lib.rt_hip_plan_fetch_full_length_step.argtypes) == 7
    m = re.search(r"^#define\s+RT_N_SCAN_MAX\s+(\d+)", raw, flags=re.M)
    assert m and int(m.group(1)) == cabi.RT_N_SCAN_MAX == 32
    for method in ("set_scan_ase_seeds", "fetch_full_length_steps", "full_length_step_ptrs", "full_length_step_tensors"):
        assert callable(getattr(backend.Plan, method)), method
    assert callable(backend.full_length_scan_loop)


class _NoNativeCalls:
    """Stands where Plan.hl stands: any use of the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the native library ({name}) before it refused its arguments")


def test_python_face_refuses_before_any_native_call(ase_small, seed_small, monkeypatch):
    p = A.base(ase_small, 2, 6)
    w, n = A.seeds_of(p)
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None          # (close() has nothing to destroy)
    plan.problem = p
    plan._n_scan_ase_seed = 0
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        plan.set_scan_ase_seeds([w] * (cabi.RT_N_SEED_MAX + 1))
    with pytest.raises(ValueError, match="not a Seed"):
        plan.set_scan_ase_seeds([w, None])
    with pytest.raises(ValueError, match="scales"):
        plan.set_scan_ase_seeds([w, n], scales=[1.0])
    with pytest.raises(AssertionError, match="native library"):    # (what is acceptable does go on to the library)
        plan.set_scan_ase_seeds([w, n], scales=[13.3, 13.3])
    assert plan.fetch_full_length_steps() == dict(ase=[], seeds=[]) and plan.full_length_step_tensors() == dict(ase=[], seeds=[])
    monkeypatch.setattr(backend.HipLibrary, "get", classmethod(lambda cls: _NoNativeCalls()))
    with pytest.raises(ValueError, match="forward method"):
        backend.full_length_scan_loop(A.base(ase_small, 1, 5), [w])
    with pytest.raises(ValueError, match="3 <= N"):
        backend.full_length_scan_loop(ls.prefix(p, 2), [w])
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        backend.full_length_scan_loop(p, [])
    with pytest.raises(ValueError, match="not a Seed"):
        backend.full_length_scan_loop(p, [w, 3.0])
    with pytest.raises(ValueError, match="scales"):
        backend.full_length_scan_loop(p, [w], scales=[1.0, 2.0])
    with pytest.raises(ValueError, match="carries a seed"):
        backend.full_length_scan_loop(ls.scan_problem(seed_small, 6), [w])
    with pytest.raises(AssertionError, match="native library"):
        backend.full_length_scan_loop(p, [w, n])
