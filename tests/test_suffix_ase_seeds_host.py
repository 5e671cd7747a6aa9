"""ASE seeds of a suffix scan (rt_hip_plan_set_suffix_ase_seeds, rt_step_rscan_ase_seeds_kernel), the parts that need no device.

1. The census of the inputs of tests/test_gpu_suffix_ase_seeds.py (tests/suffix_ase_seeds.py) on the CPU oracle, as conditions,
   so that the GPU tests cannot pass on inputs that stopped exercising what they are there for: newly escaped rays in every
   marched segment, a seed (`narrow`) whose in-range count at the exit ray differs from n to n -- a factor taken at the wrong
   state fails --, rays with all sums zero that carry a seed factor.
2. The failure matrix of the failing input, per record and n.
3. rt_hip_debug_run_shape with method 1, scan_on, use_emis, n_seed = 2 and step_on: pass kind 10, the suffix-scan march
   unchanged, the LDS of the seed-set formula with (1 + n_seed) L records.
4. Header, export map and binding carry the two symbols; the Python face refuses what it can before any native call."""
import ctypes
import fnmatch
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import ase_seeds as A
import suffix_ase_seeds as X
import suffix_scan as ss
from test_seed_scan_host import lds_by_hand

rt = importlib.import_module("raytrace-miniapp_amd")
backend = importlib.import_module("raytrace-miniapp_amd.backend")
cabi = rt.cabi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_hip.h"
NEW = ["rt_hip_plan_set_suffix_ase_seeds", "rt_hip_full_suffix_scan_loop"]


# ---------------------------------------------------------------------------------------------- 1. the census
def census(oracle, p):
    """Per n = 2 .. N: (escaped, in range of `wide` at the exit ray and not escaped, the same of `narrow`) of the suffix problem."""
    rays = p.build_rays()
    w, nr = A.seeds_of(p)
    esc, in_w, in_n = [], [], []
    for n in range(2, p.N + 1):
        pr = oracle.probe(ss.suffix(p, n), rays, want_Iv=False)
        e = (pr["flags"] & 1) != 0
        esc.append(e)
        in_w.append(int((A.in_range(w, pr["ray2"]) & ~e).sum()))
        in_n.append(int((A.in_range(nr, pr["ray2"]) & ~e).sum()))
    return rays, esc, in_w, in_n


def test_census_six_lengths(oracle, ase_small):
    p = A.base(ase_small, 1, 6)
    rays, esc, in_w, in_n = census(oracle, p)
    assert len(rays) == 1440 and len(rays) % 64 == 32 and p.beam.nv == 52 and p.method == 1
    counts = [int(e.sum()) for e in esc]
    print(f"N = 6: escaped by the end of the run of the last n = 2 .. 6 lengths: {counts}")
    assert counts == [164, 368, 522, 690, 837]
    assert counts[0] >= 20 and all(b - a >= 20 for a, b in zip(counts, counts[1:]))      # newly escaped rays in every segment
    for a, b in zip(esc, esc[1:]):
        assert not (a & ~b).any()                                                       # (escaped stays escaped)
    print(f"N = 6: in range of `wide` at the exit ray and not escaped {in_w}, of `narrow` {in_n}")
    assert in_w == [1276, 1072, 918, 750, 603]
    assert in_n == [55, 60, 49, 49, 24] and min(in_n) >= 20
    assert len(set(in_n)) >= 4                      # it differs from n to n: a factor taken at the wrong state fails
    w, nr = A.seeds_of(p)
    rows = X.problems(p, (w, nr))
    assert [len(row) for row in rows] == [5, 5, 5]
    for row in rows:
        for n, q in row.items():
            out = oracle.image_loop(q, rays)
            assert out["failure_code"] == 0, (q.label, n)                               # no failure in any of the 15 problems
            assert out["image"].any() and out["I_ang"].any(), (q.label, n)              # every record is non-zero


def test_census_two_lengths(oracle, ase_small):
    _, esc, in_w, in_n = census(oracle, A.base(ase_small, 1, 3))
    assert [int(e.sum()) for e in esc] == [164, 368] and in_n == [55, 60]


def test_census_ten_lengths(oracle, ase_small):
    _, esc, in_w, in_n = census(oracle, A.base(ase_small, 1, 10))
    print(f"N = 10: `narrow` in range and not escaped {in_n}")
    assert len(in_n) == 9 and in_n[:5] == [55, 60, 49, 49, 24] and in_n[-2:] == [14, 13] and min(in_n) >= 10


def test_census_dark_variant(oracle, ase_small):
    p = A.base(ase_small, 1, 6, dark=True)
    rays = p.build_rays()
    pr = oracle.probe(p, rays, want_Iv=False)
    assert pr["gvl"].shape[1] == 15
    zero_all = ~pr["gvl"].any(axis=1) & ~pr["evl"].any(axis=1)
    w, _ = A.seeds_of(p)
    carrying = zero_all & A.in_range(w, pr["ray2"]) & ((pr["flags"] & 1) == 0)
    print(f"dark, N = 6: all sums zero over the whole run: {int(zero_all.sum())}, in range of `wide` and not escaped {int(carrying.sum())}")
    assert int(zero_all.sum()) == 409 and int(carrying.sum()) == 96      # the marked rays carry a seed factor


# ---------------------------------------------------------------------------------------------- 2. the failure matrix
def test_failure_matrix(oracle, ase_small):
    p = A.base(ase_small, 1, 6)
    f, seeds = X.failing(p)
    rays = f.build_rays()
    rows = X.problems(f, seeds)
    got = [[oracle.image_loop(row[n], rays)["failure_code"] for n in range(2, 7)] for row in rows]
    print(f"failure matrix: {got}")
    assert got == X.WANT_CODES == [[0, 0, 0, 0, 8], [0, 0, 0, 0, 8], [4, 4, 4, 4, 12]]
    m2, m3 = [], []
    for n in range(2, 7):
        err = np.asarray(oracle.exit_rays(rows[2][n], rays)[1])
        assert not (err == -1).any()
        m2.append(int((err == -2).sum()))
        m3.append(int((err == -3).sum()))
    print(f"negated `narrow`: error -2 at n = 2 .. 6 {m2}, error -3 {m3}")
    assert m2 == [55, 60, 49, 49, 24] and m3[:4] == [0, 0, 0, 0] and m3[4] > cabi.RT_N_FAILED_MAX


# ---------------------------------------------------------------------------------------------- 3. the run shape
CU, LDS = 256, 160 * 1024
WG_WAVES = 16


def shape(**facts):
    hl = backend.HipLibrary.get()
    f = cabi.RtRunFacts(size=ctypes.sizeof(cabi.RtRunFacts), cu_count=CU, lds_limit=LDS, blob_bytes=40000, tables_bounded=1,
                        c_h3=0.025, march_prune=1, ntest_proven=1, occupancy_per_cu=1, method=1, step_on=1, scan_on=1, n_seed=2,
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
def test_shape_of_two_suffix_ase_seeds(no_knobs, one_launch):
    L = 5
    out = shape(K=52, Kp=52, n_iang=20, step_one_launch=one_launch, own_cells=1)
    assert out.kind == 0                                   # two kernels, whatever set_step_one_launch says
    assert out.pass_kind == 10 and out.pass_in_lds == 1 and out.pass_wg_waves == WG_WAVES and out.pass_grid == CU
    assert out.pass_lds == lds_by_hand(True, 20, 52, 3 * L) == 8 * (512 + 15 * (22 + 52) + 4224) <= LDS
    assert out.key_emis == 1
    # the march is the suffix-scan march unchanged: MODE 1 with the boundary stores
    assert out.mode == 1 and out.opt == 8 and out.last_march_inst == (1 | (8 << 1))
    plain = shape(K=52, Kp=52, n_iang=20, n_seed=0, step_one_launch=one_launch, own_cells=1)
    for key in ("kind", "mode", "opt", "bounded", "bthr", "grid", "chunk", "mlds", "late_chunks", "last_march_inst"):
        assert getattr(out, key) == getattr(plain, key), key
    assert plain.pass_kind == 9 and plain.pass_lds == lds_by_hand(True, 20, 52, L)     # the plain suffix scan keeps its kind
    one = shape(K=52, Kp=52, n_iang=20, n_seed=1)
    assert one.pass_kind == 10 and one.pass_lds == lds_by_hand(True, 20, 52, 2 * L)
    # the neighbours keep their kinds
    assert shape(K=52, Kp=52, n_iang=20, use_emis=0, n_seed=0).pass_kind == 9
    assert shape(K=52, Kp=52, n_iang=20, method=2).pass_kind == 8
    assert shape(K=52, Kp=52, n_iang=20, method=2, n_seed=0).pass_kind == 5
    assert shape(K=52, Kp=52, n_iang=20, scan_on=0).pass_kind == 7
    assert [n for n, _ in cabi.RtRunFacts._fields_][-1] == "scan_on"      # (no new fact)


def test_histograms_that_do_not_fit_take_global_atomics(no_knobs):
    L = 5
    assert lds_by_hand(True, 900, 84, 3 * L) <= LDS < lds_by_hand(True, 1500, 84, 3 * L)
    assert shape(K=84, Kp=84, n_iang=900).pass_in_lds == 1
    out = shape(K=84, Kp=84, n_iang=1500)
    assert out.pass_kind == 10 and out.pass_in_lds == 0 and out.pass_lds == lds_by_hand(False, 1500, 84, 3 * L) <= LDS
    assert shape(K=84, Kp=84, n_iang=1500, n_seed=0).pass_in_lds == 1      # (the plain suffix scan of these numbers keeps them)


def test_the_serial_mode_is_one_wave(no_knobs, monkeypatch):
    monkeypatch.setenv("RT_HIP_STEP_SERIAL", "1")
    out = shape(K=52, Kp=52, n_iang=20)
    assert out.pass_kind == 10 and out.pass_wg_waves == 1 and out.pass_grid == 1 and out.pass_in_lds == 1
    assert out.pass_lds == 8 * (512 + 15 * (22 + 52) + 1 * 4 * 66)
    assert out.mode == 1 and out.kind == 0


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
    assert re.search(r"int\s+rt_hip_plan_set_suffix_ase_seeds\s*\(\s*rt_hip_plan\s*\*\s*\w+,\s*int\s+n_seed,\s*const\s+rt_seed\s*\*\s*seeds,"
                     r"\s*const\s+double\s*\*\s*scales\s*\)", text)
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\s*\((.*?)\)", text, flags=re.S).group(1).split(",")]
    assert args("rt_hip_full_suffix_scan_loop") == args("rt_hip_full_length_scan_loop")
    assert list(lib.rt_hip_full_suffix_scan_loop.argtypes) == list(lib.rt_hip_full_length_scan_loop.argtypes)
    assert list(lib.rt_hip_plan_set_suffix_ase_seeds.argtypes) == list(lib.rt_hip_plan_set_scan_ase_seeds.argtypes)
    assert callable(backend.Plan.set_suffix_ase_seeds) and callable(backend.full_suffix_scan_loop)


class _NoNativeCalls:
    """Stands where Plan.hl stands: any use of the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the call reached the native library ({name}) before it refused its arguments")


def bare_plan(p, scan=True):
    plan = backend.Plan.__new__(backend.Plan)
    plan.hl = _NoNativeCalls()
    plan._h = None          # (close() has nothing to destroy)
    plan.problem = p
    plan._n_ase_seed = plan._n_scan_ase_seed = 0
    plan._scan = scan
    return plan


def test_python_face_refuses_before_any_native_call(ase_small, seed_small, monkeypatch):
    p = A.base(ase_small, 1, 6)
    w, n = A.seeds_of(p)
    plan = bare_plan(p)
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        plan.set_suffix_ase_seeds([w] * (cabi.RT_N_SEED_MAX + 1))
    with pytest.raises(ValueError, match="not a Seed"):
        plan.set_suffix_ase_seeds([w, None])
    with pytest.raises(ValueError, match="scales"):
        plan.set_suffix_ase_seeds([w, n], scales=[1.0])
    with pytest.raises(AssertionError, match="native library"):    # (what is acceptable does go on to the library)
        plan.set_suffix_ase_seeds([w, n], scales=[13.3, 13.3])
    assert plan.fetch_full_length_steps() == dict(ase=[], seeds=[]) and plan.full_length_step_tensors() == dict(ase=[], seeds=[])
    with pytest.raises(ValueError, match="suffix scan is off"):
        bare_plan(p, scan=False).set_suffix_ase_seeds([w])
    with pytest.raises(ValueError, match="backward"):
        bare_plan(A.base(ase_small, 2, 6)).set_suffix_ase_seeds([w])              # a forward plan
    with pytest.raises(ValueError, match="created with a seed"):
        bare_plan(A.carry(p, w)).set_suffix_ase_seeds([n])
    holds = bare_plan(p)
    holds._n_ase_seed = 1
    with pytest.raises(ValueError, match="holds ASE seeds"):
        holds.set_suffix_ase_seeds([w])
    monkeypatch.setattr(backend.HipLibrary, "get", classmethod(lambda cls: _NoNativeCalls()))
    with pytest.raises(ValueError, match="backward method"):
        backend.full_suffix_scan_loop(A.base(ase_small, 2, 6), [w])
    with pytest.raises(ValueError, match="forward method"):                         # (the length form keeps refusing the backward method)
        backend.full_length_scan_loop(p, [w])
    with pytest.raises(ValueError, match="3 <= N"):
        backend.full_suffix_scan_loop(ss.suffix(p, 2), [w])
    with pytest.raises(ValueError, match="RT_N_SEED_MAX"):
        backend.full_suffix_scan_loop(p, [])
    with pytest.raises(ValueError, match="not a Seed"):
        backend.full_suffix_scan_loop(p, [w, 3.0])
    with pytest.raises(ValueError, match="scales"):
        backend.full_suffix_scan_loop(p, [w], scales=[1.0, 2.0])
    with pytest.raises(ValueError, match="carries a seed"):
        backend.full_suffix_scan_loop(A.carry(p, w), [n])
    with pytest.raises(AssertionError, match="native library"):
        backend.full_suffix_scan_loop(p, [w, n])
