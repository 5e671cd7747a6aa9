"""The seeds of a length scan (rt_hip_plan_set_scan_seeds, rt_step_scan_seeds_kernel), the parts that need no device.

1. Header, binding and export map carry the four symbols; the Python face has its methods.
2. rt_hip_debug_run_shape with step_on, scan_on and n_seed > 0: pass_kind 6, the scan march unchanged, the LDS of one I_ang
   histogram and one E_v accumulator per (seed, length) -- worked out by hand from the layout
   [2 EXP_TAB | n_rec (n_ang + 3 & ~1) | n_rec Kp | 16 x 4 x 66] doubles with n_rec = n_seed L.
3. The Python face refuses what it can before any native call.
4. The census of the inputs of tests/test_gpu_seed_scan.py (tests/seed_scan.py) on the CPU oracle: in-range sets of both seeds,
   newly escaped rays per length inside either range, and both code rows of the failing input -- so that the GPU tests
   cannot pass on inputs that stopped exercising what they are there for."""
import ctypes
import fnmatch
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import length_scan as ls
import method_pairs as mp
import seed_scan as ss

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_set_scan_seeds", "rt_hip_plan_fetch_seed_length_step", "rt_hip_plan_seed_length_step_ptrs",
       "rt_hip_seed_length_scan_loop"]


# ---------------------------------------------------------------------------------------------- 1. the C ABI
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
    assert re.search(r"int\s+rt_hip_plan_set_scan_seeds\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+n_seed,\s*const\s+rt_seed\s*\*\s*seeds\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_fetch_seed_length_step\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+s,\s*int\s+n,\s*double\s*\*\s*E_v,"
                     r"\s*double\s*\*\s*nf,\s*double\s*\*\s*I_ang,\s*unsigned\s+int\s*\*\s*failure_code\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_seed_length_step_ptrs\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+s,\s*int\s+n,\s*double\s*\*\*\s*E_v_dev,"
                     r"\s*double\s*\*\*\s*nf_dev,\s*double\s*\*\*\s*iang_dev\s*\)", text)
    # the loop: rt_hip_length_scan_loop's arguments plus n_seed, seeds
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\s*\((.*?)\)", text, flags=re.S).group(1).split(",")]
    plain, mine = args("rt_hip_length_scan_loop"), args("rt_hip_seed_length_scan_loop")
    assert [a for a in mine if a not in ("n_seed", "seeds")] == plain and {"n_seed", "seeds"} <= set(mine)
    assert len(lib.rt_hip_seed_length_scan_loop.argtypes) == len(lib.rt_hip_length_scan_loop.argtypes) + 2
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"      # (the facts keep their layout)
    m = re.search(r"^#define\s+RT_N_SCAN_MAX\s+(\d+)", raw, flags=re.M)
    assert m and int(m.group(1)) == cabi.RT_N_SCAN_MAX == 32              # (stays 32 with scan seeds)
    for method in ("set_scan_seeds", "fetch_seed_length_steps", "seed_length_step_ptrs", "seed_length_step_tensors"):
        assert callable(getattr(backend.Plan, method)), method
    assert callable(backend.seed_length_scan_loop)


# ---------------------------------------------------------------------------------------------- 2. the run shape
CU, LDS = 256, 160 * 1024
EXP_TAB, XP_ROW, WG_WAVES = 256, 66, 16


def shape(**facts):
    hl = backend.HipLibrary.get()
    f = cabi.RtRunFacts(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, blob_bytes=40000, tables_bounded=1,
                        c_h3=0.025, march_prune=1, ntest_proven=1, occupancy_per_cu=1, method=2, step_on=1, scan_on=1, n_seed=2,
                        use_emis=0, n_rays=1 << 20, n_tiles=1 << 14)
    for k, v in facts.items():
        assert hasattr(f, k), k
        setattr(f, k, v)
    out = cabi.RtRunShape(size=ctypes.sizeof(cabi.RtRunShape))
    rc = hl.lib.rt_hip_debug_run_shape(ctypes.byref(f), ctypes.byref(out))
    assert rc == 0, hl.lib.rt_hip_last_error()
    return out


def lds_by_hand(in_lds, n_ang, Kp, n_rec):
    return 8 * (2 * EXP_TAB + n_rec * (((n_ang + 3) & ~1 if in_lds else 0) + Kp) + WG_WAVES * 4 * XP_ROW)


@pytest.fixture()
def no_knobs(monkeypatch):
    import os
    for k in list(os.environ):
        if k.startswith("RT_HIP_"):
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("L", [5, 19])
def test_shape_of_two_scan_seeds_on_seed_small(no_knobs, L):
    out = shape(K=84, Kp=84, n_iang=266, L=L, step_one_launch=1)
    assert out.kind == 0                                   # two kernels, whatever set_step_one_launch says
    assert out.pass_kind == 6 and out.pass_in_lds == 1 and out.pass_wg_waves == WG_WAVES and out.pass_grid == CU
    assert out.pass_lds == 8 * (512 + 2 * L * (268 + 84) + 4224) == lds_by_hand(True, 266, 84, 2 * L) <= LDS
    if L == 19:
        assert out.pass_lds == 144896
    # the march is the scan march unchanged: forward method at compile time (MODE 3), boundary stores (OPT bit 3), no pruning
    assert out.mode == 3 and out.opt == 8 and out.last_march_inst == (1 | (8 << 1)) and out.lds_tab == 1
    plain = shape(K=84, Kp=84, n_iang=266, L=L, n_seed=0)
    for key in ("mode", "opt", "bounded", "bthr", "grid", "chunk", "mlds", "late_chunks", "last_march_inst"):
        assert getattr(out, key) == getattr(plain, key), key
    assert plain.pass_kind == 5
    # one scan seed: the LDS of n_rec = L
    one = shape(K=84, Kp=84, n_iang=266, L=L, n_seed=1)
    assert one.pass_kind == 6 and one.pass_in_lds == 1 and one.pass_lds == lds_by_hand(True, 266, 84, L) == plain.pass_lds


def test_without_the_scan_a_seed_count_is_a_seed_set(no_knobs):
    out = shape(K=84, Kp=84, n_iang=266, L=5, scan_on=0)
    assert out.pass_kind == 3 and out.opt != 8
    assert shape(K=84, Kp=84, n_iang=266, L=5, scan_on=0, n_seed=0).pass_kind == 2


def test_histograms_move_to_global_memory(no_knobs):
    # 1500 cells, five lengths: the histograms fit once per length (tests/test_length_scan_host.py pins that) ...
    plain = shape(K=84, Kp=84, n_iang=1500, L=5, n_seed=0)
    assert plain.pass_kind == 5 and plain.pass_in_lds == 1
    # ... but not once per (seed, length): ten of 1502 doubles and the rest are 161 KB
    assert lds_by_hand(True, 1500, 84, 10) > LDS
    out = shape(K=84, Kp=84, n_iang=1500, L=5)
    assert out.pass_kind == 6 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 1500, 84, 10) <= LDS
    # above 32 KB of I_ang (4097 doubles) the histograms are never in LDS
    out = shape(K=84, Kp=84, n_iang=4097, L=5)
    assert out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 4097, 84, 10) <= LDS


def test_e_v_accumulators_beyond_the_limit_are_flagged(no_knobs):
    # 2 x 8 x 1024 frequencies: 128 KB of accumulators beside 37 KB of tables and rows; the shape says so, the run is RT_ERR_ARG
    # (launch_pass), as in the plain scan
    out = shape(K=1024, Kp=1024, n_iang=266, L=8)
    assert out.pass_kind == 6 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 266, 1024, 16) > LDS
    assert shape(K=1024, Kp=1024, n_iang=266, L=8, n_seed=0).pass_lds <= LDS       # (the plain scan of these numbers fits)
    assert shape(K=1024, Kp=1024, n_iang=266, L=4).pass_lds <= LDS


def test_serial_step_passes_are_one_wave_in_one_work_group(no_knobs, monkeypatch):
    """RT_HIP_STEP_SERIAL=1: every step pass as one work-group of one wave (sums in a fixed order); the march, the histograms'
    place and everything without the knob stay."""
    monkeypatch.setenv("RT_HIP_STEP_SERIAL", "1")
    for facts, kind, n_rec in ((dict(), 6, 10), (dict(n_seed=0), 5, 5), (dict(scan_on=0), 3, 2)):
        out = shape(K=84, Kp=84, n_iang=266, L=5, **facts)
        assert out.pass_kind == kind and out.pass_wg_waves == 1 and out.pass_grid == 1 and out.pass_in_lds == 1
        assert out.pass_lds == 8 * (2 * EXP_TAB + n_rec * (268 + 84) + 1 * 4 * XP_ROW)
        assert out.mode == (3 if facts.get("scan_on", 1) else out.mode) and out.kind == 0
    plain = shape(K=84, Kp=84, n_iang=266, L=5, scan_on=0, n_seed=0)
    assert plain.pass_kind == 2 and plain.pass_wg_waves == 1 and plain.pass_grid == 1
    assert shape(K=84, Kp=84, n_iang=266, L=5, scan_on=0, n_seed=0, step_on=0).pass_wg_waves == WG_WAVES    # (not the frequency kernel)
    monkeypatch.delenv("RT_HIP_STEP_SERIAL")
    assert shape(K=84, Kp=84, n_iang=266, L=5).pass_wg_waves == WG_WAVES and shape(K=84, Kp=84, n_iang=266, L=5).pass_grid == CU


# ---------------------------------------------------------------------------------------------- 3. the Python face
class _NoNativeCalls:
    """Stands where Plan.hl stands: any use of the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the native library ({name}) before it refused its arguments")


def _bare_plan(problem):
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None          # (close() has nothing to destroy)
    plan.problem = problem
    return plan


def test_set_scan_seeds_refuses_in_python_before_any_native_call(seed_small):
    six = ls.scan_problem(seed_small, 6)
    sd = six.seed
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        _bare_plan(six).set_scan_seeds([sd] * (cabi.RT_N_SEED_MAX + 1))
    for junk in ([None], [sd, "seed"], [six], [1.0]):
        with pytest.raises(ValueError, match="not a Seed"):
            _bare_plan(six).set_scan_seeds(junk)
    for ok in ([], [sd], [sd, ss.primed(sd)]):
        with pytest.raises(AssertionError, match="native library"):     # (what is acceptable does go on to the library)
            _bare_plan(six).set_scan_seeds(ok)
    plan = _bare_plan(six)
    assert plan.fetch_seed_length_steps() == [] and plan.seed_length_step_tensors() == []    # (no scan seeds: nothing to ask for)


def test_seed_length_scan_loop_refuses_in_python(ase_small, seed_small, monkeypatch):
    monkeypatch.setattr(backend.HipLibrary, "get", classmethod(lambda cls: _NoNativeCalls()))
    six = ls.scan_problem(seed_small, 6)
    with pytest.raises(ValueError, match="forward method"):
        backend.seed_length_scan_loop(mp.seed_backward(six), [six.seed])
    with pytest.raises(ValueError, match="forward method"):
        backend.seed_length_scan_loop(ase_small, [six.seed])
    with pytest.raises(ValueError, match="3 <= N"):
        backend.seed_length_scan_loop(problem_mod.prefix_lengths(seed_small, 2), [seed_small.seed])
    with pytest.raises(ValueError, match="3 <= N"):
        backend.seed_length_scan_loop(ls.scan_problem(seed_small, cabi.RT_N_SCAN_MAX + 2, scale_g0=False), [seed_small.seed])
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        backend.seed_length_scan_loop(six, [six.seed] * 3)
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        backend.seed_length_scan_loop(six, [])
    with pytest.raises(ValueError, match="not a Seed"):
        backend.seed_length_scan_loop(six, [six.seed, None])
    with pytest.raises(AssertionError, match="native library"):
        backend.seed_length_scan_loop(six, [six.seed, ss.primed(six.seed)])


# ---------------------------------------------------------------------------------------------- 4. the census of the inputs
def test_census_p450(oracle, seed_small):
    pa, pb = ss.p450(seed_small)
    assert pa.N == pb.N == 6 and pa.method == 2 and pa.gain is pb.gain and pa.beam is pb.beam
    rays = pa.build_rays()
    assert len(rays) == 450 and len(rays) % 64 != 0
    ina, inb = ss.in_range(pa.seed, rays), ss.in_range(pb.seed, rays)
    assert not np.array_equal(pa.seed.f[4], pb.seed.f[4]) and pa.seed.f0 != pb.seed.f0
    esc = ss.escaped(oracle, pa, rays)
    new = {n: esc[n] & ~esc[n - 1] for n in range(3, 7)}
    print(f"P450: in range of A {int(ina.sum())}, of B {int(inb.sum())}, of both {int((ina & inb).sum())}; escaped at n = 2 .. 6 "
          f"{[int(esc[n].sum()) for n in range(2, 7)]}; newly escaped inside A {[int((new[n] & ina).sum()) for n in range(3, 7)]}, "
          f"inside B {[int((new[n] & inb).sum()) for n in range(3, 7)]}")
    assert int(ina.sum()) == 450 and int(inb.sum()) == 96 and int((ina & inb).sum()) == 96 and not np.array_equal(ina, inb)
    assert [int(esc[n].sum()) for n in range(2, 7)] == [0, 0, 5, 15, 44]
    assert [int((new[n] & ina).sum()) for n in (4, 5, 6)] == [5, 10, 29]
    assert [int((new[n] & inb).sum()) for n in (5, 6)] == [3, 9]
    for p in (pa, pb):
        assert [oracle.image_loop(ls.prefix(p, n), rays)["failure_code"] for n in range(2, 7)] == [0] * 5


def test_census_p450_ten_lengths(oracle, seed_small):
    pa, pb = ss.p450(seed_small, 10)
    assert pa.N == pb.N == 10 and pa.n_rays_total == 450
    rays = pa.build_rays()
    for p in (pa, pb):
        assert [oracle.image_loop(ls.prefix(p, n), rays)["failure_code"] for n in (2, 6, 10)] == [0, 0, 0]


def test_census_p1350(oracle, seed_small):
    p0, p1 = ss.p1350(seed_small)
    rays = p0.build_rays()
    assert len(rays) == 1350 and p0.N == 6 and p0 is ls.seeded_forward(seed_small)
    assert ss.in_range(p0.seed, rays).all() and ss.in_range(p1.seed, rays).all()
    esc = ss.escaped(oracle, p0, rays)
    new = [int((esc[n] & ~esc[n - 1]).sum()) for n in range(3, 7)]
    print(f"P1350: escaped at n = 2: {int(esc[2].sum())}; newly escaped at n = 3 .. 6: {new}")
    assert int(esc[2].sum()) == 0 and new == [6, 55, 46, 63]      # every record needs its own boundary state


def test_census_f1350(oracle, seed_small):
    f0, f1 = ss.f1350(seed_small)
    rays = f0.build_rays()
    e0, e1 = ss.error_counts(oracle, f0, rays), ss.error_counts(oracle, f1, rays)
    print(f"F1350 / seed 0: {[e0[n] for n in range(2, 7)]}")
    print(f"F1350 / seed 1: {[e1[n] for n in range(2, 7)]}")
    assert [e0[n][0] for n in range(2, 7)] == [0, 0, 8, 8, 8]
    assert [e0[n][1][-3] for n in range(2, 7)] == [0, 0, 60, 60, 60] and all(e0[n][1][-2] == 0 for n in e0)
    assert [e1[n][0] for n in range(2, 7)] == [4, 4, 12, 12, 12]
    assert [e1[n][1][-2] for n in range(2, 7)] == [1350, 1344, 1289, 1243, 1180]
    assert all(e[n][1][-1] == 0 for e in (e0, e1) for n in e)
    # more failing rays under (seed 1, n = 2) than the report holds: the first of them in list order
    assert len(oracle.image_loop(ls.prefix(f1, 2), rays)["failed_rays"]) == cabi.RT_N_FAILED_MAX
