"""The seeds of a suffix scan (rt_hip_plan_set_suffix_seeds, rt_step_rscan_seeds_kernel): the step record of every seed beam
of the run of the LAST n lengths, n = 2 .. N, from ONE backward march of a seeded plan.

Inputs: tests/suffix_seeds.py -- suffix_scan.seeded_backward(seed_small, N), 1 350 rays (21 tiles and a ragged one of 6), nv 82;
seed 0 the problem's own, seed 1 the primed `narrow` profile.  Their census is asserted on the CPU oracle by
tests/test_suffix_seeds_host.py.

References: record (s, n) -- the oracle on the suffix problem of the last n lengths created with seed s, reduced
(backend.step_outputs_from_image), and record n of a backward suffix-scan plan created with seed s.
Gates (tests/element_gate.py, `gate_step` of tests/test_gpu_step.py): against the oracle TIGHT_TIER (1e-11 per element; the
gain-only mode) and the whole-array rel-L2 at the same tier; between two device runs "reordering".  The figures are printed
before every assertion (ELEMENT_PARITY_FILE appends them to a file: profiles/suffix_seeds_parity.txt)."""
import importlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import length_scan as ls
import suffix_scan as ss
import suffix_seeds as X
import table_variants as tv
from element_gate import TIGHT_TIER, counts_from_oracle
from test_gpu_record_refusals import BAD_N, NO_SCAN_SEED, PAIRS, Caller, access_refused, block_layout, serves
from test_gpu_step import gate_step, reduced, same_step_outputs_in_a_failing_run

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

KEYS = ("E_v", "nf", "I_ang")


# ---------------------------------------------------------------------------------------------- helpers
_refs, _plans, _kept = {}, {}, {}


def oracle_record(hip, oracle, q, rays, key=None):
    """(reduced oracle outputs, counts, the oracle's own result) of problem q, on its ray grid or on `rays`, once per session.
    (The counts are taken from the rays themselves, also for the grid: without a list counts_from_oracle has a closed form for
    the backward method that holds on the BEAM's grid, and a seeded problem's rays lie on the seed beam's -- it would count 266
    rays per pixel where 1 350 rays exist, and widen the reordering gate.)"""
    k = (id(q), key)
    if k not in _refs:
        listed = grid_rays(q) if rays is None else rays
        ora = oracle.image_loop(q, listed)
        _refs[k] = (q, reduced(hip, q, ora), counts_from_oracle(oracle, q, listed), ora)
    return _refs[k][1:]


def set_rays(plan, rays):
    return plan.set_ray_grid() if rays is None else plan.set_rays(rays)


def grid_rays(p):
    if ("rays", id(p)) not in _kept:
        _kept[("rays", id(p))] = (p, p.build_rays())
    return _kept[("rays", id(p))][1]


def run_seeds(plan, seeds, rays):
    set_rays(plan, rays).enable_step().enable_suffix_scan().set_suffix_seeds(seeds).run()
    return plan.fetch_seed_length_steps(), plan.fetch()


def two_seed_run(hip, p, seeds, rays, key):
    """The records of the two-seed install on p, once per session: (curves, fetch)."""
    k = ("two", id(p), key)
    if k not in _plans:
        with hip.Plan(p) as plan:
            _plans[k] = (p, seeds) + run_seeds(plan, list(seeds), rays)
    return _plans[k][2:]


def single_seed_scan(hip, p, seed, rays, key):
    """The records of a backward suffix-scan plan created with `seed` (no seeds installed), once per session."""
    k = ("single", id(p), id(seed), key)
    if k not in _plans:
        with hip.Plan(X.carry(p, seed)) as plan:
            set_rays(plan, rays).enable_step().enable_suffix_scan().run()
            _plans[k] = (p, seed, plan.fetch_length_steps())
    return _plans[k][2]


def same_bits(a, b, label):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (label, key)


def whole_array(rec, ref, what):
    """The whole-array gate of the gain-only mode: rel-L2 of every output within TIGHT_TIER."""
    for key in KEYS:
        nr = np.linalg.norm(ref[key])
        err = np.linalg.norm(rec[key] - ref[key]) / nr if nr > 0 else np.linalg.norm(rec[key])
        print(f"{what} / {key}: rel-L2 {err:.3e}")
        assert err <= TIGHT_TIER, (what, key, err)


def gate_all(hip, oracle, p, seeds, rays, curves, info, label, key=None):
    """Every record (s, n): its code and elements against the oracle on its reference problem."""
    rows = X.problems(p, seeds)
    N = p.N
    assert len(curves) == len(seeds) == len(rows), label
    assert info["stats"]["cell_steps"] == oracle_record(hip, oracle, rows[0][N], rays, key)[2]["counters"]["cell_steps"], label   # one march
    code = 0
    for s, (row, curve) in enumerate(zip(rows, curves)):
        assert [rec["n"] for rec in curve] == list(range(2, N + 1)), (label, s)
        for rec in curve:
            n, q = rec["n"], row[rec["n"]]
            ref, counts, ora = oracle_record(hip, oracle, q, rays, key)
            what = f"{label} / record ({s}, {n})"
            print(f"{what}: failure_code {rec['failure_code']} (oracle {ora['failure_code']})")
            assert rec["failure_code"] == ora["failure_code"], what
            code |= rec["failure_code"]
            assert rec["E_v"].any() and rec["nf"].any() and rec["I_ang"].any(), what
            gate_step(rec, ref, q, counts, TIGHT_TIER, f"{what} against the oracle")
            whole_array(rec, ref, f"{what} against the oracle")
    assert info["failure_code"] == code, label


# ---------------------------------------------------------------------------------------------- 1. parity, N = 6
@pytest.mark.parametrize("mode", ["grid", "list"])
def test_every_record_against_the_oracle(hip, oracle, seed_small, mode):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    rays = None if mode == "grid" else grid_rays(p)
    N, L, b = p.N, p.N - 1, p.beam
    with hip.Plan(p) as plan:
        curves, info = run_seeds(plan, list(seeds), rays)
        assert info["failure_code"] == 0 and len(info["failed_rays"]) == 0 and info["stats"]["n_rays"] == 1350
        assert plan.last_fused() is False and plan.last_march_instance() & (8 << 1)      # the scan instance of the march
        # the existing fetchers serve seed 0's curve, fetch_step and fetch record (0, N)
        plain = plan.fetch_length_steps()
        assert len(plain) == L and len(curves) == 2
        for a, c in zip(plain, curves[0]):
            assert a["n"] == c["n"] and a["failure_code"] == c["failure_code"]
            same_bits(a, c, f"fetch_length_steps / n = {a['n']}")
        same_bits(plan.fetch_step(), curves[0][-1], "fetch_step")
        assert np.array_equal(info["I_ang"], curves[0][-1]["I_ang"])
        assert plan.step_ptrs() == plan.seed_length_step_ptrs(0, N)[:2]
        views = plan.seed_length_step_tensors()
        assert [len(v) for v in views] == [L, L]
        for curve, vs in zip(curves, views):
            for rec, v in zip(curve, vs):
                assert v["n"] == rec["n"] and v["E_v"].shape == (b.nv,) and v["nf"].shape == (b.ny, b.nx) and v["I_ang"].shape == (b.nb, b.na)
                for key in KEYS:
                    assert np.array_equal(v[key].cpu().numpy().reshape(-1), rec[key]), (rec["n"], key)
    for i in range(L):
        assert not np.array_equal(curves[0][i]["E_v"], curves[1][i]["E_v"])
    _plans.setdefault(("two", id(p), mode), (p, seeds, curves, info))
    gate_all(hip, oracle, p, seeds, rays, curves, info, f"N = 6, ray {mode}", key=mode)


# ---------------------------------------------------------------------------------------------- 2. against single-seed plans
@pytest.mark.parametrize("mode", ["grid", "list"])
def test_each_curve_against_a_plan_created_with_that_seed(hip, oracle, seed_small, mode):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    rays = None if mode == "grid" else grid_rays(p)
    curves, _ = two_seed_run(hip, p, seeds, rays, mode)
    rows = X.problems(p, seeds)
    for s, seed in enumerate(seeds):
        parent = single_seed_scan(hip, p, seed, rays, mode)
        assert len(parent) == len(curves[s]) == p.N - 1
        for rec, ref in zip(curves[s], parent):
            q = rows[s][rec["n"]]
            assert rec["n"] == ref["n"] and rec["failure_code"] == ref["failure_code"] == 0
            gate_step(rec, ref, q, oracle_record(hip, oracle, q, rays, mode)[1], "reordering",
                      f"ray {mode} / record ({s}, {rec['n']}) against a suffix-scan plan created with the seed")


# ---------------------------------------------------------------------------------------------- 3. the smallest and an odd scan
def test_two_lengths_one_partial_chunk(hip, oracle, seed_small):
    p = ss.seeded_backward(seed_small, 3)
    seeds = X.seeds_of(p, seed_small)
    with hip.Plan(p) as plan:
        curves, info = run_seeds(plan, list(seeds), None)
    assert [len(c) for c in curves] == [2, 2]
    gate_all(hip, oracle, p, seeds, None, curves, info, "N = 3, ray grid")


def test_nine_lengths(hip, oracle, seed_small):
    p = ss.seeded_backward(seed_small, 10)
    seeds = X.seeds_of(p, seed_small)
    with hip.Plan(p) as plan:
        curves, info = run_seeds(plan, list(seeds), None)
    assert [len(c) for c in curves] == [9, 9] and info["stats"]["n_escaped"] == 302
    gate_all(hip, oracle, p, seeds, None, curves, info, "N = 10, ray grid")


# ---------------------------------------------------------------------------------------------- 4. bit for bit, one wave
_CHILD = r"""
import importlib, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import suffix_scan as ss
import suffix_seeds as X
rt = importlib.import_module("raytrace-miniapp_amd")
hip = importlib.import_module("raytrace-miniapp_amd.backend")
seed_small = rt.datfile.load(sys.argv[3])
p = ss.seeded_backward(seed_small, 6)
seeds = list(X.seeds_of(p, seed_small))
def plain_scan():
    with hip.Plan(p) as fresh:
        fresh.set_ray_grid().enable_step().enable_suffix_scan().run()
        return fresh.fetch_length_steps()
scan1, scan2 = plain_scan(), plain_scan()
with hip.Plan(p) as plan:
    plan.set_ray_grid().enable_step().enable_suffix_scan().set_suffix_seeds(seeds).run()
    two = plan.fetch_seed_length_steps()
    row0 = plan.fetch_length_steps()
    plan.run()
    two_again = plan.fetch_seed_length_steps()
    plan.set_suffix_seeds(seeds[1:]).run()
    one = plan.fetch_seed_length_steps()
    plan.set_suffix_seeds([]).run()
    back = plan.fetch_length_steps()
    assert plan.fetch_seed_length_steps() == []
assert len(back) == len(scan1) == len(row0) == 5 and len(one) == 1 and len(two) == 2
for key in ("E_v", "nf", "I_ang"):
    for i, (a, b, c) in enumerate(zip(scan1, scan2, back)):
        assert a[key].any() and two[1][i][key].any(), key
        assert np.array_equal(a[key], b[key]), ("two plain suffix-scan plans", key)
        assert np.array_equal(c[key], a[key]), ("set_suffix_seeds([]) against a plain suffix-scan plan", key)
        assert np.array_equal(two[0][i][key], two_again[0][i][key]) and np.array_equal(two[1][i][key], two_again[1][i][key]), ("two runs", key)
        assert np.array_equal(one[0][i][key], two[1][i][key]), ("a one-seed install of seed 1 against row 1 of the two-seed install", key)
        assert np.array_equal(row0[i][key], two[0][i][key]), ("fetch_length_steps against row 0", key)
        assert not np.array_equal(two[0][i][key], two[1][i][key]), key
print("SAME BITS")
"""


def test_bit_for_bit_in_the_serial_mode(seed_small):
    """RT_HIP_STEP_SERIAL=1 (every step pass as one wave: sums in a fixed order), in a child process."""
    root = Path(__file__).resolve().parents[1]
    env = dict(os.environ, RT_HIP_STEP_SERIAL="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, str(root), str(root / "tests"), str(root / "tests" / "golden" / "seed_small.dat.xz")],
                         env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "SAME BITS" in out.stdout


# ---------------------------------------------------------------------------------------------- 5. the failure matrix
@pytest.mark.parametrize("mode", ["grid", "list"])
def test_failures_per_seed_and_n(hip, oracle, seed_small, mode):
    p = ss.seeded_backward(seed_small, 6)
    f, seeds = X.failing(p, seed_small)
    rays = grid_rays(f)
    rows = X.problems(f, seeds)
    oras = [{n: oracle_record(hip, oracle, row[n], rays, "failing")[2] for n in range(2, 7)} for row in rows]
    assert [[o[n]["failure_code"] for n in range(2, 7)] for o in oras] == X.WANT_CODES
    # the rays that fail with -2 / -3 under any (seed, n), in list order: the report holds the first RT_N_FAILED_MAX
    if "fails" not in _kept:
        fails = np.zeros(len(rays), dtype=bool)
        for row in rows:
            for n in range(2, 7):
                err = np.asarray(oracle.exit_rays(row[n], rays)[1])
                assert not (err == -1).any()
                fails |= (err == -2) | (err == -3)
        _kept["fails"] = fails
    fails = _kept["fails"]
    assert int(fails.sum()) > cabi.RT_N_FAILED_MAX
    with hip.Plan(f) as plan:
        curves, info = run_seeds(plan, list(seeds), None if mode == "grid" else rays)
        again = plan.fetch_seed_length_steps()       # a second fetch serves the repeated run, it does not repeat again
        assert plan.fetch()["failure_code"] == 12
    got = [[r["failure_code"] for r in curve] for curve in curves]
    print(f"failure matrix, ray {mode}: codes {got}, fetch {info['failure_code']}, reported rays {len(info['failed_rays'])}")
    assert got == X.WANT_CODES == [[0, 0, 0, 0, 8], [4, 4, 4, 4, 12]] and info["failure_code"] == 12
    # each failing ray once, the first RT_N_FAILED_MAX of them in list order
    assert len(info["failed_rays"]) == cabi.RT_N_FAILED_MAX
    assert info["failed_rays"].tobytes() == rays[fails][:cabi.RT_N_FAILED_MAX].tobytes()
    for ca, cb in zip(again, curves):
        for ra, rb in zip(ca, cb):
            assert ra["failure_code"] == rb["failure_code"]
            same_bits(ra, rb, f"second fetch / n = {ra['n']}")
    # record (0, n), n < N, does not see seed 1's failures: the passing plan's record of seed 0
    clean_seeds = X.seeds_of(p, seed_small)
    clean, _ = two_seed_run(hip, p, clean_seeds, None if mode == "grid" else grid_rays(p), mode)
    clean_rows = X.problems(p, clean_seeds)
    for rec, ref in zip(curves[0][:-1], clean[0][:-1]):
        q = clean_rows[0][rec["n"]]
        gate_step(rec, ref, q, oracle_record(hip, oracle, q, None if mode == "grid" else grid_rays(p), mode)[1], "reordering",
                  f"failure matrix, ray {mode} / record (0, {rec['n']}) against the passing plan's")
    for s, row in enumerate(rows):
        for rec in curves[s]:
            n, q = rec["n"], row[rec["n"]]
            what = f"failure matrix, ray {mode} / record ({s}, {n})"
            assert np.isfinite(rec["E_v"]).all() and np.isfinite(rec["nf"]).all() and np.isfinite(rec["I_ang"]).all(), what
            ref, counts, _ = oracle_record(hip, oracle, q, rays, "failing")
            if s == 0:
                gate_step(rec, ref, q, counts, TIGHT_TIER, f"{what} against the oracle's reduction of the failing run")
            else:            # a negative f[4] entry is no non-negative input: the whole-array rule
                print(f"{what} against the oracle's reduction of the failing run")
                same_step_outputs_in_a_failing_run(rec, ref)


# ---------------------------------------------------------------------------------------------- 6. table updates, the scan off
def test_table_updates_keep_the_seeds_and_the_scan_off_drops_them(hip, oracle, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    N = p.N
    if ("tables_b", id(p)) not in _kept:
        _kept[("tables_b", id(p))] = tv.tables_b(p)
    pb = _kept[("tables_b", id(p))]
    with hip.Plan(p) as plan:
        first, _ = run_seeds(plan, list(seeds), None)
        # an accepted update keeps the seeds: the records on the new tables
        plan.update_gain(pb.gain).run()
        new, info = plan.fetch_seed_length_steps(), plan.fetch()
        assert len(new) == 2 and not np.array_equal(new[1][0]["E_v"], first[1][0]["E_v"])
        gate_all(hip, oracle, pb, seeds, None, new, info, "after update_gain (tables B)")
        # a refused one (a NaN in n) leaves the plan, its seeds and the records of its last run as they were
        with pytest.raises(hip.RayTraceError):
            plan.update_gain(tv.crafted_nan_index(pb, i=2).gain)
        for ca, cb in zip(plan.fetch_seed_length_steps(), new):
            for ra, rb in zip(ca, cb):
                assert ra["failure_code"] == rb["failure_code"]
                same_bits(ra, rb, f"after a refused update / n = {ra['n']}")
        plan.run()
        kept, info = plan.fetch_seed_length_steps(), plan.fetch()
        gate_all(hip, oracle, pb, seeds, None, kept, info, "a run after the refused update (tables B)")
        # the scan off drops the seeds: a plain step plan; on again, the scan is plain
        plan.enable_suffix_scan(False).run()
        assert plan.fetch_seed_length_steps() == []
        step = plan.fetch_step()
        q = X.problems(pb, seeds)[0][N]
        ref, counts, _ = oracle_record(hip, oracle, q, None)
        gate_step(step, ref, q, counts, TIGHT_TIER, "enable_suffix_scan(False): the plain step record against the oracle")
        plan.enable_suffix_scan().run()
        assert plan.fetch_seed_length_steps() == [] and len(plan.fetch_length_steps()) == N - 1
        access_refused(plan, "seed_length_step", (0, 2), PAIRS["seed_length_step"][1])


# ---------------------------------------------------------------------------------------------- 7. the step history
def test_history_files_every_record(hip, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    L = p.N - 1
    with hip.Plan(p) as plan:
        set_rays(plan, None).enable_step().enable_suffix_scan().set_suffix_seeds(list(seeds))
        plan.enable_history(2)
        filed = []
        for step in range(2):
            plan.run()
            filed.append(plan.fetch_seed_length_steps())
            plan.history_append(step)
        hist = plan.fetch_history()
        assert plan.history_info() == dict(n_steps=2, n_rec=2 * L, n_filled=2) and len(hist) == 2 * L
        for step in range(2):
            for s, curve in enumerate(filed[step]):
                for i, rec in enumerate(curve):
                    h = hist[s * L + i]
                    assert list(h["filled"]) == [1, 1] and h["failure_code"][step] == rec["failure_code"] == 0
                    for k in KEYS:
                        assert rec[k].any() and np.array_equal(h[k][step], rec[k]), (step, s, rec["n"], k)


# ---------------------------------------------------------------------------------------------- 8. the layout
def test_blocks_and_strides(hip, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    N, L, b = p.N, p.N - 1, p.beam
    with hip.Plan(p) as plan:
        run_seeds(plan, list(seeds), None)
        nf_off, ang_off, stride = block_layout(b)
        base = plan.seed_length_step_ptrs(0, 2)
        assert base[0] % 256 == 0 and base == (base[0], base[0] + nf_off, base[0] + ang_off)
        for s in range(2):
            for n in range(2, N + 1):
                ptrs = plan.seed_length_step_ptrs(s, n)
                assert ptrs == tuple(x + (s * L + n - 2) * stride for x in base), (s, n)       # block s L + n - 2 of one allocation
                if s == 0:
                    assert ptrs == plan.length_step_ptrs(n)
        both = {(s, n): s * L + n - 2 for s in range(2) for n in range(2, N + 1)}
        serves(plan, "seed_length_step", both)                  # the fetch is a read of those pointers
        serves(plan, "length_step", {(n,): n - 2 for n in range(2, N + 1)})


# ---------------------------------------------------------------------------------------------- 9. the host-pointer loop, the shapes
def test_seed_suffix_scan_loop_equals_the_plans_records(hip, oracle, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    rays = grid_rays(p)
    curves, info = two_seed_run(hip, p, seeds, rays, "list")
    out = hip.seed_suffix_scan_loop(p, list(seeds), rays)
    assert out["failure_code"] == info["failure_code"] == 0 and len(out["failed_rays"]) == 0
    assert [len(c) for c in out["records"]] == [5, 5]
    for k in ("cell_steps", "n_rays", "n_escaped", "n_skipped"):
        assert out["stats"][k] == info["stats"][k], k
    rows = X.problems(p, seeds)
    for s, (mine, theirs) in enumerate(zip(out["records"], curves)):
        for a, c in zip(mine, theirs):
            assert a["n"] == c["n"] and a["failure_code"] == c["failure_code"]
            q = rows[s][a["n"]]
            gate_step(a, c, q, oracle_record(hip, oracle, q, rays, "list")[1], "reordering",
                      f"rt_hip_seed_suffix_scan_loop / record ({s}, {a['n']}) against the plan's record")
    # the forward sibling keeps refusing the backward method, this one refuses the forward method (the C ABI itself)
    lib = hip.HipLibrary.get().lib
    forward = ls.seeded_forward(seed_small)
    for entry, q in (("seed_length_scan_loop", p), ("seed_suffix_scan_loop", forward)):
        with pytest.raises(hip.RayTraceError):
            hip._host_loop("rt_hip_" + entry, q, q.build_rays()[:64], 0, (2, q.N - 1), list(seeds))
        assert b"method" in lib.rt_hip_last_error()


def test_the_march_is_the_plain_suffix_scans_and_the_run_is_two_kernels(hip, oracle, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    seeds = X.seeds_of(p, seed_small)
    with hip.Plan(p) as plan:
        set_rays(plan, None).enable_step().enable_suffix_scan().run()
        plain_inst, plain_steps = plan.last_march_instance(), plan.fetch()["stats"]["cell_steps"]
        plan.set_suffix_seeds(list(seeds)).set_step_one_launch(True).run()       # (one launch: accepted and ignored)
        info = plan.fetch()
        assert plan.last_march_instance() == plain_inst and plain_inst & (8 << 1)
        # two kernels: not the one-launch form, both phases timed, and the ray-steps of ONE march of the N lengths
        assert plan.last_fused() is False
        march_ms, freq_ms = plan.kernel_times()
        assert march_ms > 0 and freq_ms > 0
        assert info["stats"]["cell_steps"] == plain_steps
        q = X.problems(p, seeds)[0][p.N]
        assert plain_steps == oracle_record(hip, oracle, q, None, "grid")[2]["counters"]["cell_steps"]


# ---------------------------------------------------------------------------------------------- 10. refusals, by full text
def test_refusals_through_the_c_abi(hip, ase_small, seed_small):
    p = ss.seeded_backward(seed_small, 6)
    s0, s1 = X.seeds_of(p, seed_small)
    N, ns = p.N, 2
    who = "rt_hip_plan_set_suffix_seeds"
    forward = ls.seeded_forward(seed_small)
    with hip.Plan(forward) as plan:                                       # a forward plan, its length scan off or on
        plan.enable_step()
        c = Caller(plan, [s0, s1])
        c.refuses(c.set("suffix_seeds"), who + ": the plan's method is not 1 (a forward plan takes rt_hip_plan_set_scan_seeds)")
        plan.enable_length_scan()
        c.refuses(c.set("suffix_seeds"), who + ": the plan's method is not 1 (a forward plan takes rt_hip_plan_set_scan_seeds)")
    emission = ss.emission_backward(ase_small, 6)
    with hip.Plan(emission) as plan:                                      # a plan created without a seed
        plan.enable_step().enable_suffix_scan()
        c = Caller(plan, [])
        c.refuses(c.set("suffix_seeds", 0), who + ": the plan was created without a seed (an emission plan takes rt_hip_plan_set_suffix_ase_seeds)")
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_step()
        c = Caller(plan, [s0, s1])
        for n_seed in (0, ns):                                             # the suffix scan off
            c.refuses(c.set("suffix_seeds", n_seed), who + ": the suffix scan is off (rt_hip_plan_enable_suffix_scan first)")
        c.ok(c.enable("suffix_scan"))
        c.validates("suffix_seeds")
        c.ok(c.set("suffix_seeds"))
        c.validates("suffix_seeds")                                        # (a rejected call leaves the installed seeds as they were)
        # the neighbours refuse as they did
        c.refuses(c.set("seeds"), "rt_hip_plan_set_seeds: the suffix scan is on (a seed set and a suffix scan exclude each other)")
        c.refuses(c.set("scan_seeds"), "rt_hip_plan_set_scan_seeds: the suffix scan is on (it takes no scan seeds)")
        c.refuses(c.set("suffix_ase_seeds"), "rt_hip_plan_set_suffix_ase_seeds: the plan was created with a seed (the ASE record needs an emission plan)")
        plan.run()
        # (installed through the raw C ABI: the accessors of the C ABI say what the run left -- both seeds' curves)
        serves(plan, "seed_length_step", {(s, n): s * (N - 1) + n - 2 for s in range(ns) for n in range(2, N + 1)})
        for pair in ("full_step", "full_length_step", "seed_step"):
            n_index, text = PAIRS[pair]
            access_refused(plan, pair, (0, 2)[:n_index], text)
        for index, text in (((-1, 2), NO_SCAN_SEED), ((ns, 2), NO_SCAN_SEED), ((0, 1), BAD_N), ((0, N + 1), BAD_N)):
            access_refused(plan, "seed_length_step", index, text)
        for index in ((1,), (N + 1,)):
            access_refused(plan, "length_step", index, BAD_N)
