"""ASE seeds of a suffix scan (rt_hip_plan_set_suffix_ase_seeds, rt_step_rscan_ase_seeds_kernel): the ASE record and the
records of the seed beams of the run of the LAST n lengths, n = 2 .. N, from ONE backward march.

Inputs: tests/suffix_ase_seeds.py -- ase_seeds.base(ase_small, 1, N, dark), 1 440 rays (22 tiles and a ragged one of 32 rays),
the seeds `wide` and `narrow`; their census is asserted on the CPU oracle by tests/test_suffix_ase_seeds_host.py.

References: record (0, n) -- the oracle on the suffix problem of the last n lengths, reduced (backend.step_outputs_from_image),
and record n of a plain emission suffix-scan plan; record (1 + s, n) -- the oracle on that suffix problem created with seed s,
whose scale da db the tests pass as scales[s], and record n of a backward suffix-scan plan created from carry(p, seed_s).
Gates (tests/element_gate.py, `gate_step` of tests/test_gpu_step.py): against the oracle TIGHT_TIER for the seed records and for
exact emission, DEFAULT_TIER for default emission; between two device runs "reordering".  The figures are printed before every
assertion (ELEMENT_PARITY_FILE appends them to a file: profiles/suffix_ase_seeds_parity.txt)."""
import ctypes as C
import importlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ase_seeds as A
import scan_ase_seeds as XS
import suffix_ase_seeds as X
import suffix_scan as ss
import table_variants as tv
from element_gate import DEFAULT_TIER, TIGHT_TIER, counts_from_oracle
from test_gpu_step import gate_step, reduced, same_step_outputs_in_a_failing_run

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

KEYS = ("E_v", "nf", "I_ang")


# ---------------------------------------------------------------------------------------------- helpers
_refs, _plans, _kept = {}, {}, {}


def oracle_record(hip, oracle, q, rays, key=None):
    """(reduced oracle outputs, counts, the oracle's own result) of problem q, on its ray grid or on `rays`, once per session."""
    k = (id(q), key)
    if k not in _refs:
        ora = oracle.image_loop(q, q.build_rays() if rays is None else rays)
        _refs[k] = (q, reduced(hip, q, ora), counts_from_oracle(oracle, q, rays), ora)
    return _refs[k][1:]


def set_rays(plan, rays):
    return plan.set_ray_grid() if rays is None else plan.set_rays(rays)


def curves_of(full):
    return [full["ase"]] + full["seeds"]


def grid_rays(p):
    if ("rays", id(p)) not in _kept:
        _kept[("rays", id(p))] = (p, p.build_rays())
    return _kept[("rays", id(p))][1]


def run_full_scan(plan, p, seeds, rays, exact=False):
    set_rays(plan, rays).enable_step().enable_suffix_scan()
    if exact:
        plan.set_exact_emission(True)
    plan.set_suffix_ase_seeds(seeds, X.scales_of(p, seeds))
    plan.run()
    return plan.fetch_full_length_steps(), plan.fetch()


def emission_scan(hip, p, rays, key, exact=False):
    """The records of a plain emission suffix-scan plan of p, once per session."""
    k = ("ase", id(p), key, exact)
    if k not in _plans:
        with hip.Plan(p) as plan:
            set_rays(plan, rays).enable_step().enable_suffix_scan()
            if exact:
                plan.set_exact_emission(True)
            plan.run()
            _plans[k] = (p, plan.fetch_length_steps())
    return _plans[k][1]


def seeded_scan(hip, p, seed, rays, key):
    """The records of a backward suffix-scan plan created from carry(p, seed), once per session."""
    k = ("seed", id(p), id(seed), key)
    if k not in _plans:
        with hip.Plan(A.carry(p, seed)) as plan:
            set_rays(plan, rays).enable_step().enable_suffix_scan().run()
            _plans[k] = (p, seed, plan.fetch_length_steps())
    return _plans[k][2]


def same_bits(a, b, label):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (label, key)


def gate_all(hip, oracle, p, seeds, rays, full, info, label, key=None, tier0=DEFAULT_TIER, exact=False, plans=True):
    """Every record (r, n): its code and elements against the oracle on its reference problem, and against the parents' plans."""
    curves = curves_of(full)
    rows = X.problems(p, seeds)
    N = p.N
    assert len(curves) == 1 + len(seeds) == len(rows), label
    assert info["stats"]["cell_steps"] == oracle_record(hip, oracle, rows[0][N], rays, key)[2]["counters"]["cell_steps"], label   # one march
    code = 0
    for r, (row, curve) in enumerate(zip(rows, curves)):
        assert [rec["n"] for rec in curve] == list(range(2, N + 1)), (label, r)
        parent = None
        if plans:
            parent = emission_scan(hip, p, rays, key, exact) if r == 0 else seeded_scan(hip, p, seeds[r - 1], rays, key)
        for i, rec in enumerate(curve):
            n, q = rec["n"], row[rec["n"]]
            ref, counts, ora = oracle_record(hip, oracle, q, rays, key)
            what = f"{label} / record ({r}, {n})"
            print(f"{what}: failure_code {rec['failure_code']} (oracle {ora['failure_code']})")
            assert rec["failure_code"] == ora["failure_code"], what
            code |= rec["failure_code"]
            assert rec["E_v"].any() and rec["nf"].any() and rec["I_ang"].any() == ref["I_ang"].any(), what
            gate_step(rec, ref, q, counts, tier0 if r == 0 else TIGHT_TIER, f"{what} against the oracle")
            if plans:
                gate_step(rec, parent[i], q, counts, "reordering",
                          f"{what} against a plain emission suffix-scan plan" if r == 0 else f"{what} against a suffix-scan plan created with the seed")
    assert info["failure_code"] == code, label


# ---------------------------------------------------------------------------------------------- 1. parity, N = 6
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("mode", ["grid", "list"])
def test_every_record_against_the_oracle_and_the_parents_plans(hip, oracle, ase_small, mode, exact):
    p = A.base(ase_small, 1, 6)
    seeds = A.seeds_of(p)
    rays = None if mode == "grid" else grid_rays(p)
    N, L, b = p.N, p.N - 1, p.beam
    label = f"N = 6, ray {mode}{', exact emission' if exact else ''}"
    with hip.Plan(p) as plan:
        full, info = run_full_scan(plan, p, list(seeds), rays, exact=exact)
        curves = curves_of(full)
        assert info["failure_code"] == 0 and len(info["failed_rays"]) == 0 and info["stats"]["n_rays"] == 1440
        assert plan.last_fused() is False and plan.last_march_instance() & (8 << 1)      # the scan instance of the march
        # the existing fetchers serve the ASE curve, fetch_step and fetch record (0, N)
        plain = plan.fetch_length_steps()
        assert len(plain) == L
        for a, c in zip(plain, curves[0]):
            assert a["n"] == c["n"] and a["failure_code"] == c["failure_code"]
            same_bits(a, c, f"fetch_length_steps / n = {a['n']}")
        same_bits(plan.fetch_step(), curves[0][-1], "fetch_step")
        assert np.array_equal(info["I_ang"], curves[0][-1]["I_ang"])
        assert plan.step_ptrs() == plan.full_length_step_ptrs(0, N)[:2]
        # the blocks: 3 L equal strides of one allocation, record (r, n) = block r L + (n - 2)
        base = plan.full_length_step_ptrs(0, 2)
        stride = plan.full_length_step_ptrs(0, 3)[0] - base[0]
        assert stride > 0 and stride % 256 == 0 and stride >= 8 * (b.nv + b.nx * b.ny + b.na * b.nb)
        for r in range(3):
            for n in range(2, N + 1):
                ptrs = plan.full_length_step_ptrs(r, n)
                assert ptrs == tuple(x + (r * L + n - 2) * stride for x in base), (r, n)
                if r == 0:
                    assert ptrs == plan.length_step_ptrs(n)
        views = plan.full_length_step_tensors()
        assert len(views["ase"]) == L and [len(v) for v in views["seeds"]] == [L, L]
        for curve, vs in zip(curves, curves_of(views)):
            for rec, v in zip(curve, vs):
                assert v["n"] == rec["n"] and v["E_v"].shape == (b.nv,) and v["nf"].shape == (b.ny, b.nx) and v["I_ang"].shape == (b.nb, b.na)
                for key in KEYS:
                    assert np.array_equal(v[key].cpu().numpy().reshape(-1), rec[key]), (rec["n"], key)
        # the fetchers of the neighbours refuse such a run
        lib, h = plan.hl.lib, plan._h
        assert lib.rt_hip_plan_fetch_full_step(h, 0, None, None, None, None) == cabi.RT_ERR_ARG
        assert lib.rt_hip_plan_fetch_seed_length_step(h, 0, 2, None, None, None, None) == cabi.RT_ERR_ARG
    for r in range(3):
        for i in range(L):
            for o in range(r + 1, 3):
                assert not np.array_equal(curves[r][i]["E_v"], curves[o][i]["E_v"])
    gate_all(hip, oracle, p, seeds, rays, full, info, label, key=mode, tier0=TIGHT_TIER if exact else DEFAULT_TIER, exact=exact)


# ---------------------------------------------------------------------------------------------- 2. the smallest and an odd scan
def test_two_lengths_one_partial_chunk(hip, oracle, ase_small):
    p = A.base(ase_small, 1, 3)
    seeds = A.seeds_of(p)
    with hip.Plan(p) as plan:
        full, info = run_full_scan(plan, p, list(seeds), None)
    assert [len(c) for c in curves_of(full)] == [2, 2, 2]
    gate_all(hip, oracle, p, seeds, None, full, info, "N = 3, ray grid")


def test_nine_lengths(hip, oracle, ase_small):
    p = A.base(ase_small, 1, 10)
    seeds = A.seeds_of(p)
    with hip.Plan(p) as plan:
        full, info = run_full_scan(plan, p, list(seeds), None)
    assert [len(c) for c in curves_of(full)] == [9, 9, 9] and info["stats"]["n_escaped"] == 1096
    gate_all(hip, oracle, p, seeds, None, full, info, "N = 10, ray grid")


# ---------------------------------------------------------------------------------------------- 3. the dark variant
@pytest.mark.parametrize("mode", ["grid", "dark rays first"])
def test_rays_with_all_sums_zero_stay_in_the_seed_records(hip, oracle, ase_small, mode):
    """The emission march marks a ray whose sums over the whole N-run are all zero (n_skipped): it is left out of the ASE
    records and stays in the seed records.  As a list with the marked rays first, the first six tiles hold marked rays only:
    they skip the emission half."""
    p = A.base(ase_small, 1, 6, dark=True)
    seeds = A.seeds_of(p)
    rays = None
    if mode != "grid":
        if ("dark", id(p)) not in _kept:
            grid = p.build_rays()
            pr = oracle.probe(p, grid, want_Iv=False)
            zero_all = ~pr["gvl"].any(axis=1) & ~pr["evl"].any(axis=1)
            assert int(zero_all.sum()) == 409
            _kept[("dark", id(p))] = np.ascontiguousarray(grid[XS.dark_first(zero_all)])
        rays = _kept[("dark", id(p))]
    with hip.Plan(p) as plan:
        full, info = run_full_scan(plan, p, list(seeds), rays)
    print(f"dark, {mode}: n_skipped {info['stats']['n_skipped']}")
    assert info["stats"]["n_skipped"] == 409
    gate_all(hip, oracle, p, seeds, rays, full, info, f"dark, N = 6, {mode}", key=mode)


# ---------------------------------------------------------------------------------------------- 4. the failure matrix
@pytest.mark.parametrize("mode", ["grid", "list"])
def test_failures_per_record_and_n(hip, oracle, ase_small, mode):
    p = A.base(ase_small, 1, 6)
    f, seeds = X.failing(p)
    rays = grid_rays(f)
    rows = X.problems(f, seeds)
    oras = [{n: oracle.image_loop(row[n], rays) for n in range(2, 7)} for row in rows]
    assert [[o[n]["failure_code"] for n in range(2, 7)] for o in oras] == X.WANT_CODES
    # the rays that fail with -2 / -3 under any (record, n), in list order: the report holds the first RT_N_FAILED_MAX
    fails = np.zeros(len(rays), dtype=bool)
    for row in rows:
        for n in range(2, 7):
            err = np.asarray(oracle.exit_rays(row[n], rays)[1])
            assert not (err == -1).any()
            fails |= (err == -2) | (err == -3)
    assert int(fails.sum()) > cabi.RT_N_FAILED_MAX
    with hip.Plan(f) as plan:
        full, info = run_full_scan(plan, f, list(seeds), None if mode == "grid" else rays)
        again = plan.fetch_full_length_steps()       # a second fetch serves the repeated run, it does not repeat again
        assert plan.fetch()["failure_code"] == 12
    curves = curves_of(full)
    got = [[r["failure_code"] for r in curve] for curve in curves]
    print(f"failure matrix, ray {mode}: codes {got}, fetch {info['failure_code']}, reported rays {len(info['failed_rays'])}")
    assert got == X.WANT_CODES and info["failure_code"] == 12
    assert len(info["failed_rays"]) == cabi.RT_N_FAILED_MAX
    assert info["failed_rays"].tobytes() == rays[fails][:cabi.RT_N_FAILED_MAX].tobytes()
    for ca, cb in zip(curves_of(again), curves):
        for ra, rb in zip(ca, cb):
            assert ra["failure_code"] == rb["failure_code"]
            same_bits(ra, rb, f"second fetch / n = {ra['n']}")
    for r, row in enumerate(rows):
        for rec in curves[r]:
            n, q = rec["n"], row[rec["n"]]
            what = f"failure matrix, ray {mode} / record ({r}, {n})"
            assert np.isfinite(rec["E_v"]).all() and np.isfinite(rec["nf"]).all() and np.isfinite(rec["I_ang"]).all(), what
            ref = reduced(hip, q, oras[r][n])
            if r < 2:
                gate_step(rec, ref, q, counts_from_oracle(oracle, q, rays), DEFAULT_TIER if r == 0 else TIGHT_TIER,
                          f"{what} against the oracle's reduction of the failing run")
            else:            # a negative f[4] entry is no non-negative input: the whole-array rule
                print(f"{what} against the oracle's reduction of the failing run")
                same_step_outputs_in_a_failing_run(rec, ref)


# ---------------------------------------------------------------------------------------------- 5. life cycle
_CHILD = r"""
import importlib, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import ase_seeds as A
import suffix_ase_seeds as X
rt = importlib.import_module("raytrace-miniapp_amd")
hip = importlib.import_module("raytrace-miniapp_amd.backend")
p = A.base(rt.datfile.load(sys.argv[3]), 1, 6)
seeds = list(A.seeds_of(p))
scales = X.scales_of(p, seeds)
def plain_scan():
    with hip.Plan(p) as fresh:
        fresh.set_ray_grid().enable_step().enable_suffix_scan().run()
        return fresh.fetch_length_steps()
scan1, scan2 = plain_scan(), plain_scan()
with hip.Plan(p) as plan:
    plan.set_ray_grid().enable_step().enable_suffix_scan().set_suffix_ase_seeds(seeds, scales).run()
    two = plan.fetch_full_length_steps()
    plan.run()
    two_again = plan.fetch_full_length_steps()
    plan.set_suffix_ase_seeds(seeds[:1], scales[:1]).run()
    one = plan.fetch_full_length_steps()
    plan.set_suffix_ase_seeds([]).run()
    back = plan.fetch_length_steps()
    assert plan.fetch_full_length_steps() == dict(ase=[], seeds=[])
assert len(back) == len(scan1) == 5 and len(one["seeds"]) == 1 and len(two["seeds"]) == 2
for key in ("E_v", "nf", "I_ang"):
    for i, (a, b, c) in enumerate(zip(scan1, scan2, back)):
        assert a[key].any() and two["seeds"][0][i][key].any(), key
        assert np.array_equal(a[key], b[key]), ("two plain suffix-scan plans", key)
        assert np.array_equal(c[key], a[key]), ("set_suffix_ase_seeds([]) against a plain suffix-scan plan", key)
        assert np.array_equal(two["seeds"][0][i][key], two_again["seeds"][0][i][key]), ("two runs of the two-seed install", key)
        assert np.array_equal(one["seeds"][0][i][key], two["seeds"][0][i][key]), ("a one-seed install against record 1 of the two-seed install", key)
        assert np.array_equal(one["ase"][i][key], two["ase"][i][key]), ("the ASE curve of the one-seed and the two-seed install", key)
print("SAME BITS")
"""


def test_lifecycle(hip, oracle, ase_small):
    p = A.base(ase_small, 1, 6)
    seeds = A.seeds_of(p)
    N = p.N
    if ("tables_b", id(p)) not in _kept:
        _kept[("tables_b", id(p))] = tv.tables_b(p)
    pb = _kept[("tables_b", id(p))]
    rows = X.problems(p, seeds)
    with hip.Plan(p) as plan:
        first, _ = run_full_scan(plan, p, list(seeds), None)
        # an accepted update keeps the seeds: the records on the new tables
        plan.update_gain(pb.gain).run()
        new, info = plan.fetch_full_length_steps(), plan.fetch()
        assert not np.array_equal(new["ase"][0]["E_v"], first["ase"][0]["E_v"])
        gate_all(hip, oracle, pb, seeds, None, new, info, "after update_gain (tables B)", plans=False)
        # a refused one (a non-finite index) leaves the plan and the records of its last run as they were
        with pytest.raises(hip.RayTraceError):
            plan.update_gain(tv.crafted_nan_index(pb, i=2).gain)
        for ca, cb in zip(curves_of(plan.fetch_full_length_steps()), curves_of(new)):
            for ra, rb in zip(ca, cb):
                assert ra["failure_code"] == rb["failure_code"]
                same_bits(ra, rb, f"after a refused update / n = {ra['n']}")
        # the step history files all 3 (N - 1) records
        plan.enable_history(2)
        plan.run()
        filed = plan.fetch_full_length_steps()
        plan.history_append(1)
        hist = plan.fetch_history()
        assert plan.history_info() == dict(n_steps=2, n_rec=3 * (N - 1), n_filled=1) and len(hist) == 3 * (N - 1)
        for r, curve in enumerate(curves_of(filed)):
            for i, rec in enumerate(curve):
                h = hist[r * (N - 1) + i]
                assert list(h["filled"]) == [0, 1] and h["failure_code"][1] == rec["failure_code"] == 0
                for k in KEYS:
                    assert np.array_equal(h[k][1], rec[k]) and not h[k][0].any(), (r, rec["n"], k)
        plan.enable_history(0)
        # no seeds: a plain emission suffix-scan plan (bit for bit in the serial mode, below)
        plan.update_gain(p.gain).set_suffix_ase_seeds([]).run()
        assert plan.fetch_full_length_steps() == dict(ase=[], seeds=[])
        assert plan.hl.lib.rt_hip_plan_fetch_full_length_step(plan._h, 0, 2, None, None, None, None) == cabi.RT_ERR_ARG
        for rec, ref in zip(plan.fetch_length_steps(), emission_scan(hip, p, None, None)):
            q = rows[0][rec["n"]]
            gate_step(rec, ref, q, counts_from_oracle(oracle, q, None), "reordering",
                      f"set_suffix_ase_seeds([]) against a plain emission suffix-scan plan / n = {rec['n']}")
        # the scan off drops the seeds: a plain step plan; on again, the scan is plain
        plan.set_suffix_ase_seeds(list(seeds), X.scales_of(p, seeds)).enable_suffix_scan(False).run()
        step = plan.fetch_step()
        with hip.Plan(p) as fresh:
            fresh.set_ray_grid().enable_step().run()
            gate_step(step, fresh.fetch_step(), p, counts_from_oracle(oracle, rows[0][N], None), "reordering",
                      "enable_suffix_scan(False) against a plain step plan")
        plan.enable_suffix_scan().run()
        assert plan.fetch_full_length_steps() == dict(ase=[], seeds=[]) and len(plan.fetch_length_steps()) == N - 1
        assert plan.hl.lib.rt_hip_plan_fetch_full_length_step(plan._h, 0, 2, None, None, None, None) == cabi.RT_ERR_ARG
    # bit for bit, RT_HIP_STEP_SERIAL=1 (every step pass as one wave: sums in a fixed order), in a child process
    root = Path(__file__).resolve().parents[1]
    env = dict(os.environ, RT_HIP_STEP_SERIAL="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, str(root), str(root / "tests"), str(root / "tests" / "golden" / "ASE_small.dat.xz")],
                         env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "SAME BITS" in out.stdout


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_plan_working(hip, oracle, ase_small):
    import torch

    p = A.base(ase_small, 1, 6)
    w, n = A.seeds_of(p)
    b, N = p.beam, p.N
    ERR = cabi.RT_ERR_ARG
    keep = []
    three = (cabi.RtSeed * 3)(cabi.seed_record(w, keep), cabi.seed_record(n, keep), cabi.seed_record(w, keep))
    lib = hip.HipLibrary.get().lib

    def refused(rc, *words):
        text = lib.rt_hip_last_error()
        assert rc == ERR and all(word in text for word in words), (rc, text)

    with hip.Plan(A.base(ase_small, 2, 6)) as plan:                        # a forward plan, its length scan on or off
        plan.enable_step()
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(plan._h, 1, three, None), b"method")
        plan.enable_length_scan()
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(plan._h, 1, three, None), b"method")
    with hip.Plan(A.carry(p, w)) as seeded:                                # a plan created with a seed
        seeded.enable_step().enable_suffix_scan()
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(seeded._h, 1, three, None), b"created with a seed")
    with hip.Plan(p) as plan:                                              # the suffix scan off; ASE seeds held
        plan.enable_step()
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(plan._h, 1, three, None), b"suffix scan is off")
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(plan._h, 0, None, None), b"suffix scan is off")
        plan.set_ase_seeds([w])
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(plan._h, 1, three, None), b"suffix scan is off")
        refused(lib.rt_hip_plan_enable_suffix_scan(plan._h, 1), b"ASE seeds")
    with hip.Plan(p) as plan:
        h = plan._h
        full, info = run_full_scan(plan, p, [w, n], None)
        # the refusals of the neighbours stay
        refused(lib.rt_hip_plan_set_ase_seeds(h, 1, three, None), b"suffix scan")
        refused(lib.rt_hip_plan_set_scan_ase_seeds(h, 1, three, None), b"suffix scan")
        refused(lib.rt_hip_plan_set_scan_seeds(h, 1, three), b"without a seed")
        refused(lib.rt_hip_plan_set_seeds(h, 1, three), b"without a seed")
        refused(lib.rt_hip_plan_enable_length_scan(h, 1), b"method")
        # bad arguments leave the installed seeds as they were
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(h, 3, three, None), b"RT_N_SEED_MAX")
        assert lib.rt_hip_plan_set_suffix_ase_seeds(h, -1, three, None) == ERR
        assert lib.rt_hip_plan_set_suffix_ase_seeds(h, 2, None, None) == ERR
        short = rt.Seed(list(w.x[:4]) + [w.x[4][:-1].copy()], list(w.f[:4]) + [w.f[4][:-1].copy()], 1.0)
        wrong = (cabi.RtSeed * 2)(cabi.seed_record(w, keep), cabi.seed_record(short, keep))
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(h, 2, wrong, None), b"dim[4]")
        # r and n out of range, in both accessors
        for r, k in ((3, 2), (-1, 2), (0, 1), (0, N + 1), (2, 0), (1, -1)):
            assert lib.rt_hip_plan_fetch_full_length_step(h, r, k, None, None, None, None) == ERR, (r, k)
            assert lib.rt_hip_plan_full_length_step_ptrs(h, r, k, None, None, None) == ERR, (r, k)
        assert lib.rt_hip_plan_fetch_full_length_step(h, 2, N, None, None, None, None) == cabi.RT_OK
        assert lib.rt_hip_plan_fetch_full_step(h, 0, None, None, None, None) == ERR
        assert lib.rt_hip_plan_fetch_seed_length_step(h, 0, 2, None, None, None, None) == ERR
        # what the suffix scan refuses stays refused
        assert lib.rt_hip_plan_enable_spectra(h, 1) == ERR and lib.rt_hip_plan_enable_path(h, 1) == ERR
        dev = torch.device("cuda", 0)
        ang = torch.zeros(b.na * b.nb + 8, dtype=torch.float64, device=dev)
        refused(lib.rt_hip_plan_run(h, None, None, C.c_void_p(ang.data_ptr())), b"no image and no I_ang")
        lent = torch.zeros(b.nv + b.nx * b.ny + 64, dtype=torch.float64, device=dev)
        plan.set_step_buffers(lent.data_ptr(), lent.data_ptr() + 8 * b.nv)
        refused(lib.rt_hip_plan_run(h, None, None, None), b"lent")
        plan.set_step_buffers(0, 0)
        # ... and the plan keeps working: one launch accepted and ignored, the records those of the first run
        plan.set_step_one_launch(True).run()
        assert plan.last_fused() is False
        after = plan.fetch_full_length_steps()
        march_ms, freq_ms = plan.kernel_times()
        assert march_ms > 0 and freq_ms > 0
    rows = X.problems(p, (w, n))
    for r, curve in enumerate(curves_of(after)):
        assert len(curve) == N - 1
        for rec, ref in zip(curve, curves_of(full)[r]):
            q = rows[r][rec["n"]]
            gate_step(rec, ref, q, counts_from_oracle(oracle, q, None), "reordering", f"after the refusals / record ({r}, {rec['n']})")


# ---------------------------------------------------------------------------------------------- 7. the host-pointer loop
def test_full_suffix_scan_loop_equals_the_plans_records(hip, oracle, ase_small):
    p = A.base(ase_small, 1, 6)
    seeds = A.seeds_of(p)
    rays = grid_rays(p)
    with hip.Plan(p) as plan:
        full, info = run_full_scan(plan, p, list(seeds), rays)
    out = hip.full_suffix_scan_loop(p, list(seeds), X.scales_of(p, seeds), rays)
    assert out["failure_code"] == info["failure_code"] == 0 and len(out["failed_rays"]) == 0
    assert len(out["ase"]) == 5 and [len(c) for c in out["seeds"]] == [5, 5]
    for k in ("cell_steps", "n_rays", "n_escaped", "n_skipped"):
        assert out["stats"][k] == info["stats"][k], k
    rows = X.problems(p, seeds)
    for r, (mine, theirs) in enumerate(zip(curves_of(out), curves_of(full))):
        for a, c in zip(mine, theirs):
            assert a["n"] == c["n"] and a["failure_code"] == c["failure_code"]
            q = rows[r][a["n"]]
            gate_step(a, c, q, counts_from_oracle(oracle, q, rays), "reordering",
                      f"rt_hip_full_suffix_scan_loop / record ({r}, {a['n']}) against the plan's record")
    # scales None: the problem's scale for every curve
    unscaled = hip.full_suffix_scan_loop(p, list(seeds[:1]), None, rays)
    q = rows[1][6]
    assert np.allclose(unscaled["seeds"][0][-1]["nf"] * q.scale, full["seeds"][0][-1]["nf"] * p.scale, rtol=1e-9, atol=0.0)


# ---------------------------------------------------------------------------------------------- 8. the probe
def test_the_probe_is_that_of_the_plain_run(hip, ase_small):
    p = A.base(ase_small, 1, 6)
    seeds = A.seeds_of(p)
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_probe().enable_step().run()
        plain = plan.fetch_probe()
        plan.enable_suffix_scan().set_suffix_ase_seeds(list(seeds), X.scales_of(p, seeds)).run()
        scan = plan.fetch_probe()
    for key in ("gvl", "evl", "ivl", "ray2", "flags", "steps"):
        assert plain[key].tobytes() == scan[key].tobytes(), key
    assert (plain["flags"] & 1).any() and plain["steps"].any()
