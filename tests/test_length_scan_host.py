"""The length scan (rt_hip_plan_enable_length_scan), the parts that need no device.

1. The premise, on the CPU oracle: with the forward method the run with n lengths is a prefix of the run with N.  For
   both forward pairs at N = 6 and every n = 2 .. 6 the first 3 (n - 1) slots of gvl, evl and ivl of the N = 6 probe are
   bit-equal to the whole record of the n-run; the n = N run has the N-run's exit ray; a ray the n-run reports escaped is
   escaped in every longer run, with the exit ray frozen at the escape.  (Passes without the feature.)
2. Header, binding and export map carry the four symbols and RT_N_SCAN_MAX.
3. rt_hip_debug_run_shape with scan_on: pass_kind 5, the scan march, the LDS of one histogram and one E_v accumulator per
   length -- worked out by hand from the layout [2 EXP_TAB | L (n_ang + 3 & ~1) | L Kp | 16 x 4 x 66] doubles.
4. The Python face refuses what it can before any native call."""
import ctypes
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import length_scan as ls
import method_pairs as mp

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_enable_length_scan", "rt_hip_plan_fetch_length_step", "rt_hip_plan_length_step_ptrs", "rt_hip_length_scan_loop"]


# ---------------------------------------------------------------------------------------------- 1. the premise
@pytest.mark.parametrize("pair", ["seeded", "emission"])
def test_the_run_of_n_lengths_is_a_prefix_of_the_run_of_N(oracle, ase_small, seed_small, pair):
    if pair == "seeded":
        p = ls.scan_problem(seed_small, 6)
        rays = p.build_rays(np.arange(0, p.n_rays_total, 2601, dtype=np.int64)[:3000])
    else:
        p = ls.scan_problem(mp.ase_forward(ase_small), 6)
        rays = p.build_rays(np.arange(0, p.n_rays_total, 133, dtype=np.int64)[:3000])
    assert p.method == 2 and p.N == 6 and len(rays) == 3000
    full = oracle.probe(p, rays, want_Iv=False)
    esc_prev = np.zeros(len(rays), bool)
    ray_prev = None
    for n in range(2, 7):
        q = problem_mod.prefix_lengths(p, n)
        assert q.N == n and q.method == 2 and q.scale == p.scale and q.beam is p.beam and q.seed is p.seed
        part = oracle.probe(q, rays, want_Iv=False)
        S = 3 * (n - 1)
        for key in ("gvl", "evl", "ivl"):
            a, b = full[key][:, :S], part[key]
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (pair, n, key)
        esc = (part["flags"] & 1) != 0
        # escaped by n - 1 lengths => escaped by n lengths, with the same exit ray (frozen at the escape)
        assert not (esc_prev & ~esc).any(), (pair, n)
        if ray_prev is not None:
            assert np.array_equal(part["ray2"][esc_prev].view(np.uint32), ray_prev[esc_prev].view(np.uint32)), (pair, n)
        esc_prev, ray_prev = esc, part["ray2"]
        if n == 6:
            assert np.array_equal(part["ray2"].view(np.uint32), full["ray2"].view(np.uint32))
            assert np.array_equal(part["flags"], full["flags"]) and np.array_equal(part["err"], full["err"])


def test_prefix_lengths_refuses_other_n(seed_small):
    for n in (1, 0, -1, seed_small.N + 1, 2.0, True, None):
        with pytest.raises(ValueError, match="prefix_lengths"):
            problem_mod.prefix_lengths(seed_small, n)
    q = problem_mod.prefix_lengths(seed_small, 2)
    assert q.N == 2 and q.gain[1] is seed_small.gain[1] and seed_small.N == 3


# ---------------------------------------------------------------------------------------------- 2. the C ABI
def test_entry_points_and_the_constant_are_declared_listed_and_exported():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(rt_hip_[a-z_0-9]+)\s*\(", text))
    lib = backend.HipLibrary.get().lib
    the_map = (ROOT / "raytrace-miniapp_amd" / "csrc" / "rt_hip.map").read_text()
    exported = re.findall(r"global:\s*(.*?)local:", the_map, flags=re.S)[0].replace(";", " ").split()
    import fnmatch
    for name in NEW:
        assert name in cabi.HIP_API_SYMBOLS, name
        assert name in declared, name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
        assert getattr(lib, name).restype is ctypes.c_int, name
    m = re.search(r"^#define\s+RT_N_SCAN_MAX\s+(\d+)", raw, flags=re.M)
    assert m and int(m.group(1)) == cabi.RT_N_SCAN_MAX == 32
    assert re.search(r"int\s+rt_hip_plan_fetch_length_step\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+n,\s*double\s*\*\s*E_v,\s*double\s*\*\s*nf,"
                     r"\s*double\s*\*\s*I_ang,\s*unsigned\s+int\s*\*\s*failure_code\s*\)", text)
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"
    for method in ("enable_length_scan", "fetch_length_steps", "length_step_tensors", "length_step_ptrs"):
        assert callable(getattr(backend.Plan, method))
    assert callable(backend.length_scan_loop) and callable(problem_mod.prefix_lengths)


# ---------------------------------------------------------------------------------------------- 3. the run shape
CU, LDS = 256, 160 * 1024
EXP_TAB, XP_ROW, WG_WAVES = 256, 66, 16


def shape(**facts):
    hl = backend.HipLibrary.get()
    f = cabi.RtRunFacts(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, blob_bytes=40000, tables_bounded=1,
                        c_h3=0.025, march_prune=1, ntest_proven=1, occupancy_per_cu=1, method=2, step_on=1, scan_on=1,
                        n_rays=1 << 20, n_tiles=1 << 14)
    for k, v in facts.items():
        assert hasattr(f, k), k
        setattr(f, k, v)
    out = cabi.RtRunShape(size=ctypes.sizeof(cabi.RtRunShape))
    rc = hl.lib.rt_hip_debug_run_shape(ctypes.byref(f), ctypes.byref(out))
    assert rc == 0, hl.lib.rt_hip_last_error()
    return out


def lds_by_hand(in_lds, n_ang, Kp, L):
    return 8 * (2 * EXP_TAB + L * (((n_ang + 3) & ~1 if in_lds else 0) + Kp) + WG_WAVES * 4 * XP_ROW)


@pytest.fixture()
def no_knobs(monkeypatch):
    import os
    for k in list(os.environ):
        if k.startswith("RT_HIP_"):
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("L", [5, 19])
@pytest.mark.parametrize("emis", [0, 1])
def test_scan_shape_of_seed_small_fits(no_knobs, L, emis):
    out = shape(K=84, Kp=84, n_iang=266, L=L, use_emis=emis, step_one_launch=1)
    assert out.kind == 0                                   # two kernels, whatever set_step_one_launch says
    assert out.pass_kind == 5 and out.pass_in_lds == 1 and out.pass_wg_waves == WG_WAVES
    assert out.pass_lds == lds_by_hand(True, 266, 84, L) <= LDS
    assert out.pass_grid == CU
    # the scan march: forward method at compile time (MODE 3), boundary stores (OPT bit 3), no pruning
    assert out.mode == 3 and out.opt == 8 and out.last_march_inst == (1 | (8 << 1)) and out.lds_tab == 1
    unbounded = shape(K=84, Kp=84, n_iang=266, L=L, use_emis=emis, tables_bounded=0)
    assert unbounded.mode == 3 and unbounded.opt == 8 and unbounded.bounded == 0
    big_tables = shape(K=84, Kp=84, n_iang=266, L=L, use_emis=emis, blob_bytes=200000)
    assert big_tables.lds_tab == 0 and big_tables.mode == 3 and big_tables.opt == 8


def test_without_the_scan_nothing_changes(no_knobs):
    out = shape(K=84, Kp=84, n_iang=266, L=5, scan_on=0)
    assert out.pass_kind == 2 and out.opt != 8
    seeds = shape(K=84, Kp=84, n_iang=266, L=5, scan_on=0, n_seed=2)
    assert seeds.pass_kind == 3


def test_histograms_move_to_global_memory(no_knobs):
    # above 32 KB of I_ang (4097 doubles) the histograms are never in LDS ...
    out = shape(K=84, Kp=84, n_iang=4097, L=5)
    assert out.pass_kind == 5 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 4097, 84, 5) <= LDS
    # ... and below it they leave LDS when one per length does not fit: 19 x 1502 doubles are 228 KB
    assert lds_by_hand(True, 1500, 84, 19) > LDS
    out = shape(K=84, Kp=84, n_iang=1500, L=19)
    assert out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 1500, 84, 19) <= LDS
    out = shape(K=84, Kp=84, n_iang=1500, L=5)
    assert out.pass_in_lds == 1 and out.pass_lds == lds_by_hand(True, 1500, 84, 5) <= LDS


def test_e_v_accumulators_beyond_the_limit_are_refused(no_knobs):
    # 32 lengths x 1024 frequencies: 256 KB of accumulators; the shape says so, the run is RT_ERR_ARG (launch_pass)
    out = shape(K=1024, Kp=1024, n_iang=266, L=32)
    assert out.pass_kind == 5 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 266, 1024, 32) > LDS
    ok = shape(K=1024, Kp=1024, n_iang=266, L=8)
    assert ok.pass_lds <= LDS


# ---------------------------------------------------------------------------------------------- 4. the Python face
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


def test_enable_length_scan_refuses_in_python_before_any_native_call(ase_small, seed_small):
    six = ls.scan_problem(seed_small, 6)
    with pytest.raises(ValueError, match="forward method"):
        _bare_plan(ase_small).enable_length_scan()                                  # emission, backward: method 1
    with pytest.raises(ValueError, match="forward method"):
        _bare_plan(mp.seed_backward(six)).enable_length_scan()
    with pytest.raises(ValueError, match="N >= 3"):
        _bare_plan(problem_mod.prefix_lengths(seed_small, 2)).enable_length_scan()
    with pytest.raises(ValueError, match="RT_N_SCAN_MAX"):
        _bare_plan(ls.scan_problem(seed_small, cabi.RT_N_SCAN_MAX + 2, scale_g0=False)).enable_length_scan()
    for on in (2, -1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="True / False"):
            _bare_plan(six).enable_length_scan(on)
    for p in (six, mp.ase_forward(ase_small), ls.scan_problem(seed_small, cabi.RT_N_SCAN_MAX + 1, scale_g0=False)):
        with pytest.raises(AssertionError, match="native library"):                 # (what is acceptable does go on to the library)
            _bare_plan(p).enable_length_scan()
    with pytest.raises(AssertionError, match="native library"):                     # (switching off is never refused here)
        _bare_plan(ase_small).enable_length_scan(False)


def test_length_scan_loop_refuses_in_python(ase_small, seed_small, monkeypatch):
    monkeypatch.setattr(backend.HipLibrary, "get", classmethod(lambda cls: _NoNativeCalls()))
    with pytest.raises(ValueError, match="forward method"):
        backend.length_scan_loop(ase_small)
    with pytest.raises(ValueError, match="3 <= N"):
        backend.length_scan_loop(problem_mod.prefix_lengths(seed_small, 2))
    with pytest.raises(ValueError, match="3 <= N"):
        backend.length_scan_loop(ls.scan_problem(seed_small, cabi.RT_N_SCAN_MAX + 2, scale_g0=False))


def test_without_a_device_the_loop_raises(seed_small):
    if backend.HipLibrary.get().device_count() > 0:
        return      # (a device is present: tests/test_gpu_length_scan.py runs the loop)
    p = problem_mod.regrid_seed_beam(seed_small, nx=3, ny=2, na=2, nb=2)
    with pytest.raises(backend.RayTraceError, match="no HIP device"):
        backend.length_scan_loop(p)
