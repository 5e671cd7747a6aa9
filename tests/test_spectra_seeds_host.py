"""Spectra seeds (rt_hip_plan_set_spectra_seeds), the parts that need no device.

1. Header, binding and export map carry the five symbols; the Plan methods and the one-call forms exist.
2. rt_hip_debug_run_shape with spectra_on = 1 / 2 (spectra mode / length spectra) and n_seed = 1, 2, either method: pass kinds
   13 and 14, the march instance and pass_lds of the single-seed mode (the seeds share the one staging of a wave, so the LDS is
   the spectra pass's by the hand formula); n_seed = 0 answers as before (kinds 1 and 12).
3. The census the GPU tests rest on (tests/test_gpu_spectra_seeds.py), on the CPU oracle's probe.  Measured when the tests were
   written (clean = err 0 and a non-zero spectrum), of 1 350 rays at n = 2 .. 6:
       forward    seed 0   1350, 1344, 1289, 1243, 1180      seed 1   80 at every n (the factor is taken at the launch ray)
       backward   seed 0   1300, 1215, 1124, 1051, 967       seed 1   44, 49, 69, 61, 56 (the factor at the state that serves n)
   Asserted: at least 40 everywhere; seed 1's non-zero set differs from seed 0's at every n; backward it changes from n to
   n + 1; in the failing variants the codes differ by seed and by n.
4. The Python face refuses what it can before any native call."""
import ctypes
import fnmatch
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import spectra_seeds as S
from test_seed_scan_host import CU, EXP_TAB, LDS, WG_WAVES, no_knobs, shape  # noqa: F401  (no_knobs is a fixture)

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_set_spectra_seeds", "rt_hip_plan_fetch_seed_spectra", "rt_hip_plan_seed_spectra_ptrs",
       "rt_hip_plan_fetch_seed_length_spectra", "rt_hip_plan_seed_length_spectra_ptrs"]
XS_ROW, WAVE = 18, 64
PASS_SPEC, PASS_SPEC_SCAN, PASS_SPEC_SEEDS, PASS_SPEC_SCAN_SEEDS = 1, 12, 13, 14


# ---------------------------------------------------------------------------------------------- 1. the C ABI
def test_entry_points_are_declared_listed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(rt_hip_[a-z_0-9]+)\s*\(", text))
    lib = backend.HipLibrary.get().lib
    the_map = (ROOT / "raytrace-miniapp_amd" / "csrc" / "rt_hip.map").read_text()
    exported = re.findall(r"global:\s*(.*?)local:", the_map, flags=re.S)[0].replace(";", " ").split()
    for name in NEW:
        assert name in cabi.HIP_API_SYMBOLS, name
        assert name in declared, name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
        assert getattr(lib, name).restype is ctypes.c_int, name
    assert re.search(r"int\s+rt_hip_plan_set_spectra_seeds\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+n_seed,\s*const\s+rt_seed\s*\*\s*seeds\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_fetch_seed_spectra\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+s,\s*double\s*\*\s*Iv,\s*rt_ray\s*\*\s*ray2,"
                     r"\s*int32_t\s*\*\s*err\s*\)", text)
    assert re.search(r"int\s+rt_hip_plan_seed_length_spectra_ptrs\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+s,\s*int\s+n,\s*double\s*\*\*\s*Iv_dev,"
                     r"\s*rt_ray\s*\*\*\s*ray2_dev,\s*int32_t\s*\*\*\s*err_dev\s*\)", text)
    assert len(lib.rt_hip_plan_set_spectra_seeds.argtypes) == 3
    assert len(lib.rt_hip_plan_fetch_seed_spectra.argtypes) == 5 and len(lib.rt_hip_plan_seed_spectra_ptrs.argtypes) == 5
    assert len(lib.rt_hip_plan_fetch_seed_length_spectra.argtypes) == 6 and len(lib.rt_hip_plan_seed_length_spectra_ptrs.argtypes) == 6
    for method in ("set_spectra_seeds", "fetch_seed_spectra", "fetch_seed_length_spectra", "seed_spectra_ptrs", "seed_length_spectra_ptrs",
                   "seed_spectra_tensors", "seed_length_spectra_tensors"):
        assert callable(getattr(backend.Plan, method)), method
    assert callable(backend.calc_rays_seeds) and callable(backend.calc_rays_seeds_lengths)
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"      # (the facts keep their layout)
    assert "seed sets per length" not in HEADER.read_text()               # (the "Not built" line of length spectra has lost it)


# ---------------------------------------------------------------------------------------------- 2. the run shape
def spec_lds_by_hand():
    """The LDS of the spectra pass: the two exponent tables and [64][XS_ROW] staging doubles per wave (rt_spec.hip); the
    seeds share that one staging."""
    return 8 * (2 * EXP_TAB + WG_WAVES * WAVE * XS_ROW)


def spec_shape(**facts):
    return shape(**dict(dict(step_on=0, scan_on=0, n_seed=0, use_emis=0, n_iang=266, K=82, Kp=84), **facts))


MARCH = ("kind", "lds_tab", "n_launch", "bthr", "mode", "bounded", "opt", "last_march_inst", "mlds", "grid", "chunk", "park", "late_first",
         "late_waves", "late_chunks")


@pytest.mark.parametrize("n_seed", [1, 2])
@pytest.mark.parametrize("L", [2, 5])
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("mode", [1, 2])
def test_shape_with_spectra_seeds(no_knobs, mode, method, L, n_seed):
    """This test fails on the parent commit, which answers pass kinds 1 and 12 whatever n_seed says."""
    one = spec_shape(spectra_on=mode, method=method, L=L, n_seed=0)
    out = spec_shape(spectra_on=mode, method=method, L=L, n_seed=n_seed, step_one_launch=1)
    assert one.pass_kind == (PASS_SPEC if mode == 1 else PASS_SPEC_SCAN)                        # n_seed = 0 answers as before
    assert out.pass_kind == (PASS_SPEC_SEEDS if mode == 1 else PASS_SPEC_SCAN_SEEDS)
    assert out.kind == 0 and out.pass_in_lds == 0 and out.pass_wg_waves == WG_WAVES and out.pass_grid == CU
    assert out.pass_lds == one.pass_lds == spec_lds_by_hand() <= LDS
    for key in MARCH:                                                                           # the march instance of the single-seed mode
        assert getattr(out, key) == getattr(one, key), key
    assert bool(out.opt & 8) == (mode == 2)                                                     # the scan march exactly in length spectra
    assert out.key_s6 == (1 if L == 2 else 0) and out.key_emis == 0


def test_other_modes_keep_their_kinds_beside_n_seed(no_knobs):
    assert spec_shape(spectra_on=0, step_on=1, n_seed=2, method=2, L=5).pass_kind == 3          # a seed set in step mode
    assert spec_shape(spectra_on=0, step_on=1, scan_on=1, n_seed=2, method=2, L=5).pass_kind == 6
    assert spec_shape(spectra_on=0, step_on=1, scan_on=1, n_seed=2, method=1, L=5).pass_kind == 11
    assert spec_shape(spectra_on=0, n_seed=0, method=2, L=5).pass_kind == 0


def test_a_limit_that_is_too_small_refuses_the_pass(no_knobs):
    need = spec_lds_by_hand()
    for mode, kind in ((1, PASS_SPEC_SEEDS), (2, PASS_SPEC_SCAN_SEEDS)):
        assert spec_shape(spectra_on=mode, method=2, L=5, n_seed=2, lds_limit=need).pass_lds == need
        out = spec_shape(spectra_on=mode, method=2, L=5, n_seed=2, lds_limit=need - 8)
        assert out.pass_kind == kind and out.pass_lds == need > need - 8         # pass_lds above lds_limit: the run is refused


# ---------------------------------------------------------------------------------------------- 3. the census
@pytest.mark.parametrize("method", [1, 2])
def test_census_of_the_two_seeds(oracle, seed_small, method):
    p = S.problem_of(seed_small, method)
    rays = p.build_rays()
    seeds = S.seeds_of(p, seed_small)
    assert p.N == 6 and len(rays) == 1350 and len(rays) % 64 == 6 and p.method == method and p.beam.nv == 82
    assert not np.array_equal(seeds[0].f[4], seeds[1].f[4]) and seeds[0].f0 != seeds[1].f0
    cen = [{n: S.probe_of(oracle, S.sub(p, n), sd, rays) for n in range(2, 7)} for sd in seeds]
    nonzero = [{n: c[n]["Iv"].any(axis=1) for n in c} for c in cen]
    clean = [{n: (c[n]["err"] == 0) & nz[n] for n in c} for c, nz in zip(cen, nonzero)]
    counts = [[int(cl[n].sum()) for n in range(2, 7)] for cl in clean]
    print(f"census / method {method}: clean non-zero rows at n = 2 .. 6 per seed {counts} of {len(rays)}")
    for s in range(2):
        for n in range(2, 7):
            assert counts[s][n - 2] >= 40, (method, s, n)
            assert np.array_equal(cen[0][n]["err"] == -1, cen[s][n]["err"] == -1)               # error -1 does not depend on the seed
            assert cen[0][n]["ray2"].tobytes() == cen[s][n]["ray2"].tobytes()                   # ... nor does the exit ray
    for n in range(2, 7):
        assert not np.array_equal(nonzero[0][n], nonzero[1][n]), (method, n)                    # the seeds light different rays
        both = clean[0][n] & clean[1][n]
        assert both.any() and not np.array_equal(cen[0][n]["Iv"][both], cen[1][n]["Iv"][both])
        if method == 1 and n < 6:
            assert not np.array_equal(nonzero[1][n], nonzero[1][n + 1]), n                      # backward: seed 1's set changes with n
    assert counts == S.CLEAN_6[method], counts


@pytest.mark.parametrize("method", [1, 2])
def test_census_of_the_failing_variants(oracle, seed_small, method):
    p, seeds = S.failing(S.problem_of(seed_small, method), seed_small)
    rays = p.build_rays()
    codes = [[S.code_of(S.probe_of(oracle, S.sub(p, n), sd, rays)["err"]) for n in range(2, 7)] for sd in seeds]
    print(f"failing variant / method {method}: codes per seed at n = 2 .. 6 {codes}")
    assert codes == S.WANT_CODES[method]
    assert codes[0] != codes[1] and len(set(codes[0])) > 1 and len(set(codes[1])) > 1           # by seed and by n
    whole = [S.code_of(S.probe_of(oracle, p, sd, rays)["err"]) for sd in seeds]                 # spectra mode: the whole problem
    assert whole == [codes[0][-1], codes[1][-1]] and whole[0] != whole[1]


# ---------------------------------------------------------------------------------------------- 4. the Python face
class _NoNativeCalls:
    """Stands where Plan.hl stands: any use of the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the native library ({name}) before it refused its arguments")


def test_the_python_face_refuses_before_any_native_call(seed_small, monkeypatch):
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None
    plan.problem = seed_small
    sd = seed_small.seed
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        plan.set_spectra_seeds([sd] * (cabi.RT_N_SEED_MAX + 1))
    with pytest.raises(ValueError, match="not a Seed"):
        plan.set_spectra_seeds([sd, "seed"])
    with pytest.raises(AssertionError, match="native library"):            # (what is acceptable does go on to the library)
        plan.set_spectra_seeds([sd])
    assert plan.fetch_seed_spectra() == [] and plan.fetch_seed_length_spectra() == []           # no seeds installed: nothing to fetch
    monkeypatch.setattr(backend.HipLibrary, "get", classmethod(lambda cls: _NoNativeCalls()))
    rays = seed_small.build_rays(np.arange(4, dtype=np.int64))
    for call in (backend.calc_rays_seeds, backend.calc_rays_seeds_lengths):
        with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
            call(S.problem_of(seed_small, 2), [], rays)
        with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
            call(S.problem_of(seed_small, 2), [sd] * 3, rays)
    with pytest.raises(ValueError, match="3 <= N"):
        backend.calc_rays_seeds_lengths(S.sub(S.problem_of(seed_small, 2), 2), [sd], rays)


def test_switching_a_mode_off_forgets_the_seeds_on_the_python_face():
    class _Lib:
        def rt_hip_plan_enable_spectra(self, h, on):
            return cabi.RT_OK

        def rt_hip_plan_enable_length_spectra(self, h, on):
            return cabi.RT_OK

    class _Hl:
        lib = _Lib()

        def check(self, rc, what):
            assert rc == cabi.RT_OK, what

    plan = backend.Plan.__new__(backend.Plan)
    plan.hl, plan._h = _Hl(), None
    plan.enable_spectra(True)
    plan._n_spec_seed = 2
    plan.enable_spectra(True)
    assert plan._n_spec_seed == 2
    plan.enable_spectra(False)
    assert plan._n_spec_seed == 0
    plan.enable_length_spectra(True)
    plan._n_spec_seed = 1
    plan.enable_length_spectra(False)
    assert plan._n_spec_seed == 0
