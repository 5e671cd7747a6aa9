"""The seeds of a suffix scan (rt_hip_plan_set_suffix_seeds, rt_step_rscan_seeds_kernel), the parts that need no device.

1. The census of the inputs of tests/test_gpu_suffix_seeds.py (tests/suffix_seeds.py) on the CPU oracle, as conditions, so
   that the GPU tests cannot pass on inputs that stopped exercising what they are there for: newly escaped rays in the marched
   segments, a second seed whose in-range count at the exit ray differs from n to n -- a factor taken at the wrong state, or
   from the wrong seed's tables, fails.
2. The failure matrix of the failing input, per seed and n.
3. rt_hip_debug_run_shape with method 1, scan_on, use_emis = 0, n_seed = 2 and step_on: pass kind 11, the suffix-scan march
   unchanged, the LDS of the seed-set formula with n_seed L records.
4. Header, export map and binding carry the two symbols; the Python face refuses what it can before any native call."""
import ctypes
import fnmatch
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import length_scan as ls
import suffix_scan as ss
import suffix_seeds as X
from test_seed_scan_host import lds_by_hand

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_set_suffix_seeds", "rt_hip_seed_suffix_scan_loop"]


# ---------------------------------------------------------------------------------------------- 1. the census
def census(oracle, p, seeds):
    """Per n = 2 .. N: escaped in the run of the last n lengths; per seed: in range at the exit ray and not escaped."""
    rays = p.build_rays()
    esc, inside = [], [[] for _ in seeds]
    for n in range(2, p.N + 1):
        pr = oracle.probe(ss.suffix(p, n), rays, want_Iv=False)
        e = (pr["flags"] & 1) != 0
        esc.append(e)
        for s, seed in enumerate(seeds):
            inside[s].append(int((X.in_range(seed, pr["ray2"]) & ~e).sum()))
    return rays, esc, inside


def test_census_six_lengths(oracle, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    rays, esc, inside = census(oracle, p, seeds)
    assert len(rays) == 1350 and len(rays) % 64 == 6 and len(rays) // 64 == 21 and p.beam.nv == 82 and p.method == 1
    assert seeds[0] is p.seed and seeds[1].f[4].shape == (82,) and seeds[1].f0 != seeds[0].f0
    counts = [int(e.sum()) for e in esc]
    print(f"N = 6: escaped by the end of the run of the last n = 2 .. 6 lengths: {counts}")
    assert counts == X.ESCAPED_6 == [0, 6, 61, 107, 170]
    for a, b in zip(esc, esc[1:]):
        assert not (a & ~b).any()                                                       # (escaped stays escaped)
    print(f"N = 6: in range at the exit ray and not escaped, seed 0 {inside[0]}, seed 1 {inside[1]}")
    assert inside == X.IN_RANGE_6
    assert inside[0] == [1300, 1215, 1124, 1051, 967]
    assert inside[1] == [44, 49, 69, 61, 56] and len(set(inside[1])) == 5 and min(inside[1]) >= 20
    rows = X.problems(p, seeds)
    assert [len(row) for row in rows] == [5, 5]
    for row in rows:
        for n, q in row.items():
            out = oracle.image_loop(q, rays)
            assert out["failure_code"] == 0, (q.label, n)                               # no failure in any of the ten problems
            assert out["image"].any() and out["I_ang"].any(), (q.label, n)              # every record is non-zero


def test_census_two_lengths(oracle, seed_small):
    p = ss.seeded_backward(seed_small, 3)
    _, esc, inside = census(oracle, p, X.seeds_of(p, seed_small))
    assert inside == [[1300, 1214], [44, 49]]


def test_census_ten_lengths(oracle, seed_small):
    p = ss.seeded_backward(seed_small, 10)
    _, esc, inside = census(oracle, p, X.seeds_of(p, seed_small))
    counts = [int(e.sum()) for e in esc]
    print(f"N = 10: seed 1 in range and not escaped {inside[1]}, escaped {counts}")
    assert inside[1] == [44, 49, 69, 61, 56, 47, 46, 40, 37]
    assert counts[-1] == max(counts) == 302


# ---------------------------------------------------------------------------------------------- 2. the failure matrix
def test_failure_matrix(oracle, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    f, seeds = X.failing(p, seed_small)
    rays = f.build_rays()
    rows = X.problems(f, seeds)
    got = [[oracle.image_loop(row[n], rays)["failure_code"] for n in range(2, 7)] for row in rows]
    print(f"failure matrix: {got}")
    assert got == X.WANT_CODES == [[0, 0, 0, 0, 8], [4, 4, 4, 4, 12]]
    m2, m3 = [], []
    for s, row in enumerate(rows):
        for n in range(2, 7):
            err = np.asarray(oracle.exit_rays(row[n], rays)[1])
            assert not (err == -1).any()                                                # no error -1
            if s == 1:
                m2.append(int((err == -2).sum()))
                m3.append(int((err == -3).sum()))
    print(f"seed 1 with f[4][3] negated: error -2 at n = 2 .. 6 {m2}, error -3 {m3}")
    assert m2 == [44, 49, 69, 61, 56]
    assert m3[:4] == [0, 0, 0, 0] and m3[4] == 154 > cabi.RT_N_FAILED_MAX


# ---------------------------------------------------------------------------------------------- 3. the run shape
CU, LDS = 256, 160 * 1024
WG_WAVES = 16


def shape(**facts):
    hl = backend.HipLibrary.get()
    f = cabi.RtRunFacts(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, blob_bytes=40000, tables_bounded=1,
                        c_h3=0.025, march_prune=1, ntest_proven=1, occupancy_per_cu=1, method=1, step_on=1, scan_on=1, n_seed=2,
                        use_emis=0, L=5, n_rays=1 << 20, n_tiles=1 << 14)
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
def test_shape_of_two_suffix_seeds(no_knobs, one_launch):
    L = 5
    out = shape(K=82, Kp=84, n_iang=30, step_one_launch=one_launch)
    assert out.kind == 0                                   # two kernels, whatever set_step_one_launch says
    assert out.pass_kind == 11 and out.pass_in_lds == 1 and out.pass_wg_waves == WG_WAVES and out.pass_grid == CU
    assert out.pass_lds == lds_by_hand(True, 30, 84, 2 * L) == 8 * (512 + 10 * (32 + 84) + 4224) <= LDS
    # the march is the suffix-scan march of the seeded plan unchanged: MODE 0 with the boundary stores
    assert out.mode == 0 and out.opt == 8 and out.last_march_inst == (1 | (8 << 1))
    plain = shape(K=82, Kp=84, n_iang=30, n_seed=0, step_one_launch=one_launch)
    march = ("kind", "lds_tab", "n_launch", "bthr", "mode", "bounded", "opt", "last_march_inst", "mlds", "grid", "chunk", "park", "spin_limit",
             "no_skip", "late_first", "late_waves", "late_chunks", "occupancy_asked")
    for key in march:
        assert getattr(out, key) == getattr(plain, key), key
    assert plain.pass_kind == 9 and plain.pass_lds == lds_by_hand(True, 30, 84, L)     # the plain suffix scan keeps its kind
    one = shape(K=82, Kp=84, n_iang=30, n_seed=1)
    assert one.pass_kind == 11 and one.pass_lds == lds_by_hand(True, 30, 84, L)
    # the neighbours keep their kinds
    assert shape(K=82, Kp=84, n_iang=30, use_emis=1).pass_kind == 10
    assert shape(K=82, Kp=84, n_iang=30, use_emis=1, n_seed=0).pass_kind == 9
    assert shape(K=82, Kp=84, n_iang=30, method=2).pass_kind == 6
    assert shape(K=82, Kp=84, n_iang=30, method=2, n_seed=0).pass_kind == 5
    assert shape(K=82, Kp=84, n_iang=30, scan_on=0).pass_kind == 3
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"      # (no new fact)


def test_histograms_that_do_not_fit_take_global_atomics(no_knobs):
    L = 5
    assert lds_by_hand(True, 1500, 84, L) <= LDS < lds_by_hand(True, 1500, 84, 2 * L)
    assert shape(K=84, Kp=84, n_iang=900).pass_in_lds == 1
    out = shape(K=84, Kp=84, n_iang=1500)
    assert out.pass_kind == 11 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 1500, 84, 2 * L) <= LDS
    assert shape(K=84, Kp=84, n_iang=1500, n_seed=0).pass_in_lds == 1      # (the plain suffix scan of these numbers keeps them)


def test_the_serial_mode_is_one_wave(no_knobs, monkeypatch):
    monkeypatch.setenv("RT_HIP_STEP_SERIAL", "1")
    out = shape(K=82, Kp=84, n_iang=30)
    assert out.pass_kind == 11 and out.pass_wg_waves == 1 and out.pass_grid == 1 and out.pass_in_lds == 1
    assert out.pass_lds == 8 * (512 + 10 * (32 + 84) + 1 * 4 * 66)
    assert out.mode == 0 and out.kind == 0


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
    assert re.search(r"int\s+rt_hip_plan_set_suffix_seeds\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+n_seed,\s*const\s+rt_seed\s*\*\s*seeds\s*\)", text)
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\s*\((.*?)\)", text, flags=re.S).group(1).split(",")]
    assert args("rt_hip_seed_suffix_scan_loop") == args("rt_hip_seed_length_scan_loop")
    assert list(lib.rt_hip_seed_suffix_scan_loop.argtypes) == list(lib.rt_hip_seed_length_scan_loop.argtypes)
    assert list(lib.rt_hip_plan_set_suffix_seeds.argtypes) == list(lib.rt_hip_plan_set_scan_seeds.argtypes)
    assert callable(backend.Plan.set_suffix_seeds) and callable(backend.seed_suffix_scan_loop)


class _NoNativeCalls:
    """Stands where Plan.hl stands: any use of the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the native library ({name}) before it refused its arguments")


def bare_plan(p, scan=True):
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None          # (close() has nothing to destroy)
    plan.problem = p
    plan._scan = scan
    return plan


def test_python_face_refuses_before_any_native_call(ase_small, seed_small, monkeypatch):
    p = ss.seeded_backward(seed_small, 6)
    s0, s1 = X.seeds_of(p, seed_small)
    plan = bare_plan(p)
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        plan.set_suffix_seeds([s0] * (cabi.RT_N_SEED_MAX + 1))
    with pytest.raises(ValueError, match="not a Seed"):
        plan.set_suffix_seeds([s0, None])
    with pytest.raises(AssertionError, match="native library"):    # (what is acceptable does go on to the library)
        plan.set_suffix_seeds([s0, s1])
    assert plan.fetch_seed_length_steps() == [] and plan.seed_length_step_tensors() == []
    with pytest.raises(ValueError, match="scan is off"):
        bare_plan(p, scan=False).set_suffix_seeds([s0])
    forward = ls.seeded_forward(seed_small)
    assert forward.method == 2 and forward.seed is not None
    with pytest.raises(ValueError, match="backward"):
        bare_plan(forward).set_suffix_seeds([s0])                                  # a forward plan
    emission = ss.emission_backward(ase_small, 6)
    assert emission.seed is None and emission.method == 1
    with pytest.raises(ValueError, match="created without a seed"):
        bare_plan(emission).set_suffix_seeds([s0])
    monkeypatch.setattr(backend.HipLibrary, "get", classmethod(lambda cls: _NoNativeCalls()))
    with pytest.raises(ValueError, match="backward method"):
        backend.seed_suffix_scan_loop(forward, [s0])
    with pytest.raises(ValueError, match="forward method"):                         # (the length form keeps refusing the backward method)
        backend.seed_length_scan_loop(p, [s0])
    with pytest.raises(ValueError, match="3 <= N"):
        backend.seed_suffix_scan_loop(ss.suffix(p, 2), [s0])
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        backend.seed_suffix_scan_loop(p, [])
    with pytest.raises(ValueError, match="not a Seed"):
        backend.seed_suffix_scan_loop(p, [s0, 3.0])
    with pytest.raises(AssertionError, match="native library"):
        backend.seed_suffix_scan_loop(p, [s0, s1])
