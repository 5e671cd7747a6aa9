"""The suffix scan (rt_hip_plan_enable_suffix_scan), the parts that need no device.

1. The premise, on the CPU oracle: with the backward method the run of N lengths BEGINS with the whole run of the problem
   that holds the last n - 1 lengths (problem.suffix_lengths).  For both backward pairs at N = 6, 3000 rays each, and
   every n = 2 .. 6: gvl, evl and ivl of the suffix problem's probe are bit-equal to slots 3 (N - n) .. 3 (N - 1) - 1 of
   the full run's; the n = N run is the full run in exit ray, flags and codes; a ray the n-run reports escaped is escaped
   in every longer run.  (Passes without the feature: suffix_lengths is restated here for it.)
2. The census the GPU tests rest on (tests/suffix_scan.py), asserted by structure so that a changed helper is noticed.
   Measured on the oracle when the tests were written: emission 164 / 368 / 522 / 690 / 837 escaped rays of 1440 for
   n = 2 .. 6, every ray with a positive spectrum at every n; seeded 0 / 6 / 61 / 107 / 170 of 1350, 1300 .. 967 rays
   with a non-zero seed factor; no failing ray in either.
3. suffix_lengths refuses other n and keeps gain[0].
4. Header, binding and export map carry the two symbols; RtRunFacts still ends with scan_on.
5. rt_hip_debug_run_shape with scan_on = 1 and method = 1: pass_kind 9, two kernels, the backward scan march (MODE 1 with
   use_emis, MODE 0 without, OPT bit 3), the LDS of one histogram and one E_v accumulator per length by the hand formula
   of tests/test_seed_scan_host.py; the same facts with method = 2 are the length scan's as before.
6. The Python face refuses what it can before any native call."""
import copy
import ctypes
import fnmatch
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import length_scan as ls
import method_pairs as mp
import suffix_scan as sx
from test_seed_scan_host import CU, LDS, WG_WAVES, lds_by_hand, no_knobs, shape  # noqa: F401  (no_knobs is a fixture)

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_enable_suffix_scan", "rt_hip_suffix_scan_loop"]


def suffix_by_definition(p, n):
    """The definition (include/rt_hip.h), restated so that the premise is checked without problem.suffix_lengths."""
    q = copy.copy(p)
    q.gain = [p.gain[0]] + list(p.gain[p.N - n + 1:])
    q.golden_image = q.golden_I_ang = None
    return q


# ---------------------------------------------------------------------------------------------- 1. the premise
@pytest.mark.parametrize("pair", ["emission", "seeded"])
def test_the_run_of_N_lengths_begins_with_the_run_of_the_last_n(oracle, ase_small, seed_small, pair):
    if pair == "emission":
        p = ls.scan_problem(ase_small, 6)
        rays = p.build_rays(np.arange(0, p.n_rays_total, 133, dtype=np.int64)[:3000])
    else:
        p = ls.scan_problem(mp.seed_backward(seed_small), 6)
        rays = p.build_rays(np.arange(0, p.n_rays_total, 2601, dtype=np.int64)[:3000])
    assert p.method == 1 and p.N == 6 and len(rays) == 3000
    full = oracle.probe(p, rays, want_Iv=False)
    esc_prev = np.zeros(len(rays), bool)
    n_esc = []
    for n in range(2, 7):
        q = suffix_by_definition(p, n)
        assert q.N == n and q.method == 1 and q.gain[0] is p.gain[0] and q.gain[-1] is p.gain[-1]
        part = oracle.probe(q, rays, want_Iv=False)
        lo, hi = 3 * (p.N - n), 3 * (p.N - 1)
        for key in ("gvl", "evl", "ivl"):
            a, b = full[key][:, lo:hi], part[key]
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (pair, n, key)
        esc = (part["flags"] & 1) != 0
        assert not (esc_prev & ~esc).any(), (pair, n)          # escaped by n - 1 lengths => escaped by n
        n_esc.append(int(esc.sum()))
        esc_prev = esc
        if n == 6:
            assert np.array_equal(part["ray2"].view(np.uint32), full["ray2"].view(np.uint32))
            assert np.array_equal(part["flags"], full["flags"]) and np.array_equal(part["err"], full["err"])
    print(f"{pair}: escaped rays of the suffix runs n = 2 .. 6: {n_esc}")
    assert n_esc == sorted(n_esc) and n_esc[-1] > n_esc[0]


# ---------------------------------------------------------------------------------------------- 2. the census
def test_census_of_the_emission_problem(oracle, ase_small):
    p = sx.emission_backward(ase_small)
    rays = p.build_rays()
    assert len(rays) == 1440 and p.method == 1 and p.N == 6 and p.seed is None
    for i in range(1, 6):
        for j in range(i + 1, 6):
            assert not np.array_equal(p.gain[i].g0, p.gain[j].g0), (i, j)
    cen = sx.census(oracle, p, rays, "emission")
    esc = [int((cen[n]["flags"] & 1).astype(bool).sum()) for n in range(2, 7)]
    print(f"census / emission backward: escaped at n = 2 .. 6: {esc} of {len(rays)}")
    # every marched segment has new escapes; escaped and live rays at every n
    assert esc[0] > 0 and all(b > a for a, b in zip(esc, esc[1:])) and esc[-1] < len(rays), esc
    for n in range(2, 7):
        assert not cen[n]["err"].any(), n                                  # no failing ray
        assert (cen[n]["Iv"].max(axis=1) > 0).all(), n                     # every ray has a positive spectrum
        if n > 2:
            assert not ((cen[n - 1]["flags"] & 1).astype(bool) & ~(cen[n]["flags"] & 1).astype(bool)).any()


def test_census_of_the_seeded_problem(oracle, seed_small):
    p = sx.seeded_backward(seed_small)
    rays = p.build_rays()
    assert len(rays) == 1350 and p.method == 1 and p.N == 6 and p.seed is not None
    cen = sx.census(oracle, p, rays, "seeded")
    esc = [int((cen[n]["flags"] & 1).astype(bool).sum()) for n in range(2, 7)]
    lit = [int((cen[n]["Iv"].max(axis=1) > 0).sum()) for n in range(2, 7)]
    print(f"census / seeded backward: escaped at n = 2 .. 6: {esc}, rays with a non-zero seed factor: {lit} of {len(rays)}")
    # marched segments 2 .. 5 have new escapes, segment 1 has none; rays with and without a seed factor at every n
    assert esc[0] == 0 and all(b > a for a, b in zip(esc, esc[1:])), esc
    assert all(0 < c < len(rays) for c in lit), lit
    for n in range(2, 7):
        assert not cen[n]["err"].any(), n
        assert not cen[n]["Iv"][(cen[n]["flags"] & 1).astype(bool)].any(), n   # an escaped ray carries no seed


# ---------------------------------------------------------------------------------------------- 3. suffix_lengths
def test_suffix_lengths_refuses_other_n_and_keeps_gain_0(ase_small, seed_small):
    six = ls.scan_problem(ase_small, 6)
    for n in (1, 0, -1, 7, 2.0, True, None):
        with pytest.raises(ValueError, match="suffix_lengths"):
            problem_mod.suffix_lengths(six, n)
    for n in range(2, 7):
        q = problem_mod.suffix_lengths(six, n)
        ref = suffix_by_definition(six, n)
        assert q.N == n and len(q.gain) == n and all(a is b for a, b in zip(q.gain, ref.gain))
        assert q.gain[0] is six.gain[0] and q.gain[-1] is six.gain[-1]
        assert q.beam is six.beam and q.method == 1 and q.scale == six.scale and q.seed is six.seed
        assert q.golden_image is None and q.golden_I_ang is None and q.label.endswith(f"/ last {n} lengths")
    full = problem_mod.suffix_lengths(six, 6)
    assert all(a is b for a, b in zip(full.gain, six.gain))
    sb = mp.seed_backward(seed_small)
    assert problem_mod.suffix_lengths(sb, 2).gain == [sb.gain[0], sb.gain[2]]


# ---------------------------------------------------------------------------------------------- 4. the C ABI
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
    assert re.search(r"int\s+rt_hip_plan_enable_suffix_scan\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+on\s*\)", text)
    assert lib.rt_hip_suffix_scan_loop.argtypes == lib.rt_hip_length_scan_loop.argtypes
    for method in ("enable_suffix_scan", "fetch_length_steps", "length_step_tensors", "length_step_ptrs"):
        assert callable(getattr(backend.Plan, method))
    assert callable(backend.suffix_scan_loop) and callable(problem_mod.suffix_lengths)


def test_run_facts_still_end_with_scan_on():
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"
    raw = HEADER.read_text()
    body = re.search(r"typedef struct rt_hip_run_facts\s*\{(.*?)\}\s*rt_hip_run_facts;", raw, flags=re.S)
    if body:    # (the last member the header declares)
        members = re.findall(r"\b(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
        assert members[-1] == "scan_on"


# ---------------------------------------------------------------------------------------------- 5. the run shape
@pytest.mark.parametrize("L", [5, 19])
@pytest.mark.parametrize("emis", [0, 1])
def test_shape_of_the_suffix_scan(no_knobs, L, emis):
    out = shape(K=84, Kp=84, n_iang=266, L=L, n_seed=0, method=1, use_emis=emis, step_one_launch=1)
    assert out.kind == 0                                   # two kernels, whatever set_step_one_launch says
    assert out.pass_kind == 9 and out.pass_in_lds == 1 and out.pass_wg_waves == WG_WAVES and out.pass_grid == CU
    assert out.pass_lds == lds_by_hand(True, 266, 84, L) <= LDS
    # the backward scan march: MODE 1 (backward and emission at compile time) or MODE 0, boundary stores (OPT bit 3), no pruning
    assert out.mode == (1 if emis else 0) and out.opt == 8 and out.last_march_inst == (1 | (8 << 1)) and out.lds_tab == 1
    assert out.last_march_inst & (8 << 1)
    unbounded = shape(K=84, Kp=84, n_iang=266, L=L, n_seed=0, method=1, use_emis=emis, tables_bounded=0)
    assert unbounded.mode == (1 if emis else 0) and unbounded.opt == 8 and unbounded.bounded == 0 and unbounded.pass_kind == 9
    big_tables = shape(K=84, Kp=84, n_iang=266, L=L, n_seed=0, method=1, use_emis=emis, blob_bytes=200000)
    assert big_tables.lds_tab == 0 and big_tables.mode == (1 if emis else 0) and big_tables.opt == 8
    # an emission grid plan that would otherwise take the one launch keeps two kernels as well
    grid = shape(K=84, Kp=84, n_iang=266, L=L, n_seed=0, method=1, use_emis=emis, own_cells=1, rays_per_pixel=64, step_one_launch=1)
    assert grid.kind == 0 and grid.pass_kind == 9


def test_histograms_of_the_suffix_scan_move_to_global_memory(no_knobs):
    out = shape(K=84, Kp=84, n_iang=4097, L=5, n_seed=0, method=1, use_emis=1)
    assert out.pass_kind == 9 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 4097, 84, 5) <= LDS
    assert lds_by_hand(True, 1500, 84, 19) > LDS           # 19 histograms of 1502 doubles do not fit
    out = shape(K=84, Kp=84, n_iang=1500, L=19, n_seed=0, method=1, use_emis=1)
    assert out.pass_kind == 9 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 1500, 84, 19) <= LDS
    out = shape(K=84, Kp=84, n_iang=1500, L=5, n_seed=0, method=1, use_emis=0)
    assert out.pass_kind == 9 and out.pass_in_lds == 1 and out.pass_lds == lds_by_hand(True, 1500, 84, 5) <= LDS


@pytest.mark.parametrize("emis", [0, 1])
def test_the_same_facts_with_the_forward_method_are_the_length_scan(no_knobs, emis):
    out = shape(K=84, Kp=84, n_iang=266, L=5, n_seed=0, method=2, use_emis=emis)
    assert out.pass_kind == 5 and out.mode == 3 and out.opt == 8
    # ... and a backward plan without the scan is a plain step plan
    plain = shape(K=84, Kp=84, n_iang=266, L=5, n_seed=0, method=1, use_emis=emis, scan_on=0)
    assert plain.pass_kind == 2 and not plain.opt & 8


# ---------------------------------------------------------------------------------------------- 6. the Python face
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


def test_enable_suffix_scan_refuses_in_python_before_any_native_call(ase_small, seed_small):
    six = ls.scan_problem(ase_small, 6)
    with pytest.raises(ValueError, match="backward method"):
        _bare_plan(seed_small).enable_suffix_scan()                                   # seeded, forward: method 2
    with pytest.raises(ValueError, match="backward method"):
        _bare_plan(mp.ase_forward(six)).enable_suffix_scan()
    with pytest.raises(ValueError, match="N >= 3"):
        _bare_plan(problem_mod.suffix_lengths(ase_small, 2)).enable_suffix_scan()
    with pytest.raises(ValueError, match="RT_N_SCAN_MAX"):
        _bare_plan(ls.scan_problem(ase_small, cabi.RT_N_SCAN_MAX + 2, scale_g0=False)).enable_suffix_scan()
    for on in (2, -1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="True / False"):
            _bare_plan(six).enable_suffix_scan(on)
    for p in (six, mp.seed_backward(seed_small), ls.scan_problem(ase_small, cabi.RT_N_SCAN_MAX + 1, scale_g0=False)):
        with pytest.raises(AssertionError, match="native library"):                   # (what is acceptable does go on to the library)
            _bare_plan(p).enable_suffix_scan()


def test_suffix_scan_loop_refuses_in_python(ase_small, seed_small, monkeypatch):
    monkeypatch.setattr(backend.HipLibrary, "get", classmethod(lambda cls: _NoNativeCalls()))
    with pytest.raises(ValueError, match="backward method"):
        backend.suffix_scan_loop(seed_small)
    with pytest.raises(ValueError, match="3 <= N"):
        backend.suffix_scan_loop(problem_mod.suffix_lengths(ase_small, 2))
    with pytest.raises(ValueError, match="3 <= N"):
        backend.suffix_scan_loop(ls.scan_problem(ase_small, cabi.RT_N_SCAN_MAX + 2, scale_g0=False))
