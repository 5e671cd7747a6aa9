"""Length spectra on the GPU (rt_spec_scan_kernel, rt_hip_plan_enable_length_spectra): RayTrace::calc_ray for every ray at
every plasma length n = 2 .. N from ONE march, against the oracle's probe of the sub-problems (prefix_lengths with the
forward method, suffix_lengths with the backward one), against plain spectra-mode plans of the sub-problems, and against the
records of the scan plans on the same rays.

The problems are those of the scan tests at N = 6 (tests/length_scan.py, tests/suffix_scan.py): 1 440 rays = 22.5 tiles with
K = 52 (full groups of four frequencies) in emission mode, 1 350 rays with K = 82 (a left-over of two) in gain-only mode.
tests/test_length_spectra_host.py asserts the census these tests rest on: at every n at least 70 % of the rows are clean and
non-zero, most spectra change from n - 1 to n, and the escaped set grows.

Gates: err equal ray by ray; ray2 bit for bit where err != -1; rows that are zero on the CPU are zero here; Iv per ray within
the project's gate 1e-5 rel-L2 (test_gpu_spectra.GATE) in default emission and 1e-11 (the tight tier) in gain-only mode and
with exact emission; against a spectra-mode plan of the sub-problem bit-equal in gain-only mode and with exact emission.
Measured figures are printed before every assertion; with SPECTRA_PARITY_FILE set they are appended to that file
(profiles/length_spectra_parity.txt)."""
import dataclasses
import importlib

import numpy as np
import pytest

import length_scan as ls
import method_pairs as mp
import seed_profiles as sp
import suffix_scan as sx
import table_variants as tv
from element_gate import TIGHT_TIER, assert_elements, deposit_cells, gate_outputs, contribution_counts, reordering_tol
from test_gpu_spectra import GATE, check_against, note, ray2_bits_equal, row_figures

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

PROBLEMS = ["emission forward", "seeded forward", "emission backward", "seeded backward"]


# ---------------------------------------------------------------------------------------------- helpers
def problem_of(name, ase_small, seed_small, N=6):
    if name == "emission forward":
        return ls.emission_forward(ase_small, N)
    if name == "seeded forward":
        return ls.seeded_forward(seed_small, N)
    if name == "emission backward":
        return sx.emission_backward(ase_small, N)
    return sx.seeded_backward(seed_small, N)


def sub(p, n):
    """The sub-problem of n lengths: the first n of a forward problem, gain[0] and the last n - 1 of a backward one."""
    return ls.prefix(p, n) if p.method == 2 else sx.suffix(p, n)


def sub_new(p, n):
    return problem_mod.prefix_lengths(p, n) if p.method == 2 else problem_mod.suffix_lengths(p, n)


_refs = {}


def oracle_blocks(oracle, p, rays, key, fresh=False):
    """The oracle's probe (err, ray2, Iv, flags) of every sub-problem, computed once per key and left unchanged."""
    if key not in _refs:
        _refs[key] = {n: oracle.probe(sub_new(p, n) if fresh else sub(p, n), rays, want_Iv=True) for n in range(2, p.N + 1)}
    return _refs[key]


def run_lspec(plan, rays, exact=False, **grid):
    (plan.set_ray_grid(**grid) if rays is None else plan.set_rays(rays))
    if exact:
        plan.set_exact_emission(True)
    plan.enable_length_spectra().run()
    info = plan.fetch()
    return plan.fetch_length_spectra(), info


def spectra_plan(hip, q, rays, exact=False):
    with hip.Plan(q) as plan:
        plan.set_rays(rays)
        if exact:
            plan.set_exact_emission(True)
        return plan.enable_spectra().run().fetch_spectra()


def gate_blocks(blocks, refs, label, tight):
    """Every block against the oracle: check_against (err, ray2, zero rows, the 1e-5 gate, no clean row left out), the tight
    tier on top where it applies.  Returns the largest per-ray rel-L2."""
    worst = 0.0
    assert [b["n"] for b in blocks] == sorted(refs)
    for blk in blocks:
        ref = refs[blk["n"]]
        rows, nzero = check_against(blk, ref, f"{label} / n = {blk['n']}")
        assert rows + nzero == int((ref["err"] == 0).sum())          # no row with err = 0 in the oracle is left out
        ok = ref["err"] == 0
        l2 = row_figures(blk["Iv"][ok], ref["Iv"][ok])[0]
        worst = max(worst, l2)
        if tight:
            assert l2 < TIGHT_TIER, (label, blk["n"], l2)
    note(f"{label}: worst per-ray rel-L2 over all n {worst:.3e} ({'tight tier 1e-11' if tight else 'gate 1e-5'})")
    return worst


def codes_of(refs):
    """(the OR of the codes over all (ray, n), the rays failing under any n as a mask)."""
    code, failing = 0, None
    for n, ref in refs.items():
        for e in (-1, -2, -3):
            if (ref["err"] == e).any():
                code |= 1 << -e
        failing = (ref["err"] != 0) if failing is None else (failing | (ref["err"] != 0))
    return code, failing


def check_report(info, refs, rays, label):
    code, failing = codes_of(refs)
    want = [tuple(r) for r in rays[failing].tolist()]
    got = [tuple(r) for r in info["failed_rays"].tolist()]
    print(f"{label}: failure_code {info['failure_code']} (oracle {code}), failing rays {len(want)}, reported {len(got)}")
    assert info["failure_code"] == code, label
    if len(want) > cabi.RT_N_FAILED_MAX:      # the first RT_N_FAILED_MAX of them in list order
        assert got == want[:cabi.RT_N_FAILED_MAX], label
    else:                                     # each once, in the order the waves reached the report
        assert sorted(got) == sorted(want), label


# ---------------------------------------------------------------------------------------------- 1. every block against the oracle
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("name", PROBLEMS)
def test_every_block_against_the_oracle(hip, oracle, ase_small, seed_small, name, mode):
    p = problem_of(name, ase_small, seed_small)
    rays = p.build_rays()
    refs = oracle_blocks(oracle, p, rays, name)
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, None if mode == "grid" else rays)
        assert info["stats"]["n_rays"] == len(rays) and plan.last_fused() is False and info["image"] is None
        assert plan.last_march_instance() & (8 << 1)                    # the scan instance of the march
        march_ms, freq_ms = plan.kernel_times()
        assert march_ms > 0 and freq_ms > 0                             # two kernels: the pass is reported as freq_ms
        views = plan.length_spectra_tensors()
        L, K = p.N - 1, p.beam.nv
        assert tuple(views["Iv"].shape) == (L, len(rays), K) and tuple(views["err"].shape) == (L, len(rays))
        assert views["Iv"].data_ptr() == plan.length_spectra_ptrs(2)[0]
        assert plan.length_spectra_ptrs(3)[0] == plan.length_spectra_ptrs(2)[0] + 8 * len(rays) * K      # length-major
        iv, r2, er = views["Iv"].cpu().numpy(), views["ray2"].cpu().numpy(), views["err"].cpu().numpy()
        for j, blk in enumerate(blocks):
            assert np.array_equal(iv[j], blk["Iv"], equal_nan=True) and np.array_equal(er[j], blk["err"])
            assert np.array_equal(r2[j].view(np.uint32), cabi.rays_to_array(blk["ray2"]).astype(np.float32).view(np.uint32))
    assert len(blocks) == 5 and info["failure_code"] == 0
    gate_blocks(blocks, refs, f"length spectra / {name}, ray {mode}", tight=name.startswith("seeded"))
    for a, b in zip(blocks, blocks[1:]):      # the blocks are those of different lengths
        assert a["Iv"].any() and not np.array_equal(a["Iv"], b["Iv"])


@pytest.mark.parametrize("name", ["emission forward", "emission backward"])
def test_exact_emission_is_in_the_tight_tier(hip, oracle, ase_small, seed_small, name):
    p = problem_of(name, ase_small, seed_small)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, None, exact=True)
    assert info["failure_code"] == 0
    gate_blocks(blocks, oracle_blocks(oracle, p, rays, name), f"length spectra / {name}, exact emission", tight=True)


# ---------------------------------------------------------------------------------------------- 2. against spectra-mode plans of the sub-problems
_lspec_runs = {}


def lspec_on_the_list(hip, oracle, p, name, exact):
    """(blocks, info) of one length-spectra run on the problem's ray list, once per (name, exact); cell_steps checked."""
    if (name, exact) not in _lspec_runs:
        rays = p.build_rays()
        with hip.Plan(p) as plan:
            blocks, info = run_lspec(plan, rays, exact=exact)
        full = oracle.image_loop(p, rays)
        assert info["stats"]["cell_steps"] == full["counters"]["cell_steps"]          # the march of all N lengths, once
        _lspec_runs[(name, exact)] = (blocks, info)
    return _lspec_runs[(name, exact)]


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("name,exact", [(n, False) for n in PROBLEMS] + [("emission forward", True), ("emission backward", True)])
def test_a_block_against_a_spectra_plan_of_the_sub_problem(hip, oracle, ase_small, seed_small, name, exact, n):
    """Bit-equal in gain-only mode and with exact emission, within the gate in default emission.

    n = 3 is the case that tells: the plan of the N = 3 sub-problem takes the SF = 6 instance of rt_spec_kernel, whose small-|gl|
    update is contracted otherwise than the SF = 0 instance's; rows integrated in the SF = 0 form differed there in 3 088 (forward)
    and 3 093 (backward) of 74 880 elements by one unit in the last place, and with exact emission the kernel integrates the
    rows of n = 3 in the SF = 6 form (AseUpdate::apply_n3, rt_spec_scan.hip)."""
    p = problem_of(name, ase_small, seed_small)
    rays = p.build_rays()
    blocks, _ = lspec_on_the_list(hip, oracle, p, name, exact)
    blk = blocks[n - 2]
    assert blk["n"] == n
    one = spectra_plan(hip, sub(p, n), rays, exact=exact)
    label = f"length spectra / {name}{', exact emission' if exact else ''} / n = {n} against a spectra plan of the sub-problem"
    assert np.array_equal(blk["err"], one["err"]) and ray2_bits_equal(blk["ray2"], one["ray2"], one["err"] != -1), label
    if exact or name.startswith("seeded"):
        diff = blk["Iv"].view(np.uint64) != one["Iv"].view(np.uint64)
        nz = one["Iv"] != 0
        rel = float((np.abs(blk["Iv"] - one["Iv"])[nz] / np.abs(one["Iv"])[nz]).max()) if nz.any() else 0.0
        note(f"{label}: differing elements {int(diff.sum())} of {diff.size} in {int(diff.any(axis=1).sum())} rows, max rel diff {rel:.3e}")
        assert not diff.any(), label
    else:
        l2, el, rows, nzero = row_figures(blk["Iv"], one["Iv"])
        note(f"{label}: rows {rows} (+{nzero} zero rows), max per-ray rel-L2 {l2:.3e}, max per-element rel diff {el:.3e}")
        assert l2 < GATE, (label, l2)


# ---------------------------------------------------------------------------------------------- 3. codes that depend on n
def failing_variant(clean, which):
    """failing_variant of tests/test_gpu_suffix_scan.py, restated: a failing table at length 3 of 5 -- read by the suffixes
    of n >= 4 lengths and by the prefixes of n >= 4 lengths, not by n = 2, 3."""
    if which == "nan":
        return tv.crafted_nan_lineshape(clean, i=3)
    gains = list(clean.gain)        # a negative lineshape table, one length only
    gains[3] = dataclasses.replace(clean.gain[3], gv=-clean.gain[3].gv)
    return tv.with_gain(clean, gains, " negative gv at length 3")


@pytest.mark.parametrize("name,which", [("seeded backward", "nan"), ("emission backward", "nan"), ("emission backward", "negative"),
                                        ("seeded forward", "nan"), ("emission forward", "nan"), ("emission forward", "negative")])
def test_codes_that_depend_on_n(hip, oracle, ase_small, seed_small, name, which):
    clean = problem_of(name, ase_small, seed_small)
    p = failing_variant(clean, which)
    rays = p.build_rays()
    refs = oracle_blocks(oracle, p, rays, (name, which), fresh=True)
    per_n = {n: sorted(set(refs[n]["err"].tolist())) for n in refs}
    print(f"{name} / {which}: oracle codes per n {per_n}")
    assert not refs[2]["err"].any() and not refs[3]["err"].any()          # the failing table is not read yet
    assert any(refs[n]["err"].any() for n in (4, 5, 6))
    for mode_rays in (None, rays):
        with hip.Plan(p) as plan:
            blocks, info = run_lspec(plan, mode_rays)
        for blk in blocks:
            ref = refs[blk["n"]]
            check_against(blk, ref, f"length spectra / {name} / {which}, {'grid' if mode_rays is None else 'list'} / n = {blk['n']}")
        check_report(info, refs, rays, f"length spectra / {name} / {which}")


@pytest.mark.parametrize("name", PROBLEMS)
def test_a_steep_list_ray_fails_under_every_n(hip, oracle, ase_small, seed_small, name):
    """One ray launched almost perpendicular to z (s.z^2 < 0.01, Helper.h:515): error -1 under every n, reported once."""
    p = problem_of(name, ase_small, seed_small)
    bad = p.build_rays().copy()
    bad["a"][7] = 1500.0
    refs = oracle_blocks(oracle, p, bad, (name, "steep"))
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, bad)
    for blk in blocks:
        ref = refs[blk["n"]]
        assert ref["err"][7] == -1 and blk["err"][7] == -1 and not blk["Iv"][7].any()
        assert all(blk["ray2"][k][7] == 0 for k in "xyab")
        check_against(blk, ref, f"length spectra / {name}, a steep ray / n = {blk['n']}")
    assert info["failure_code"] == 1 << 1 and len(info["failed_rays"]) == 1 and info["failed_rays"][0] == bad[7]


# ---------------------------------------------------------------------------------------------- 4. shapes at which the kernel can go wrong
@pytest.mark.parametrize("name", PROBLEMS)
def test_three_lengths_one_boundary(hip, oracle, ase_small, seed_small, name):
    """N = 3: one boundary, less than any chunk."""
    p = problem_of(name, ase_small, seed_small, N=3)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, None)
    assert len(blocks) == 2 and info["failure_code"] == 0
    gate_blocks(blocks, oracle_blocks(oracle, p, rays, (name, 3)), f"length spectra / {name}, N = 3", tight=name.startswith("seeded"))


@pytest.mark.parametrize("method", [1, 2])
def test_ten_lengths_ragged_tile_seeded(hip, oracle, seed_small, method):
    """N = 10 on 450 rays: nine blocks are several chunks, the last tile holds two rays."""
    key = ("lspec e2e10", method)
    if key not in ls._built:
        base = mp.seed_backward(seed_small) if method == 1 else seed_small
        ls._built[key] = ls.scan_problem(sp.e2e_problem(base, "limiter"), 10)
    p = ls._built[key]
    assert p.n_rays_total == 450 and p.N == 10 and p.method == method
    rays = p.build_rays()
    refs = oracle_blocks(oracle, p, rays, key)
    for mode_rays in (None, rays):
        with hip.Plan(p) as plan:
            blocks, info = run_lspec(plan, mode_rays)
        assert len(blocks) == 9 and info["stats"]["n_rays"] == 450
        gate_blocks(blocks, refs, f"length spectra / seeded, method {method}, N = 10, 450 rays, {'grid' if mode_rays is None else 'list'}", tight=True)
        check_report(info, refs, rays, f"length spectra / seeded, method {method}, N = 10")


@pytest.mark.parametrize("name", ["emission forward", "emission backward"])
def test_ten_lengths_ragged_tile_emission(hip, oracle, ase_small, seed_small, name):
    """N = 10 in emission mode on 130 rays of the grid: two tiles and a last tile of two rays, three chunks of suffixes."""
    p = problem_of(name, ase_small, seed_small, N=10)
    rays = p.build_rays(np.arange(5, 5 + 11 * 130, 11, dtype=np.int64))
    assert len(rays) == 130
    refs = oracle_blocks(oracle, p, rays, (name, 10))
    for exact in (False, True):
        with hip.Plan(p) as plan:
            blocks, info = run_lspec(plan, rays, exact=exact)
        assert len(blocks) == 9
        gate_blocks(blocks, refs, f"length spectra / {name}, N = 10, 130 rays{', exact emission' if exact else ''}", tight=exact)
        check_report(info, refs, rays, f"length spectra / {name}, N = 10")


@pytest.mark.parametrize("name", PROBLEMS)
def test_one_ray(hip, oracle, ase_small, seed_small, name):
    p = problem_of(name, ase_small, seed_small)
    rays = p.build_rays()[611:612].copy()
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, rays)
    assert info["stats"]["n_rays"] == 1
    gate_blocks(blocks, oracle_blocks(oracle, p, rays, (name, "one ray")), f"length spectra / {name}, one ray", tight=name.startswith("seeded"))


@pytest.mark.parametrize("name,nv", [("emission forward", 51), ("seeded forward", 81), ("emission backward", 51), ("seeded backward", 81)])
def test_an_odd_number_of_frequencies(hip, oracle, ase_small, seed_small, name, nv):
    """An odd K: no 16-byte store is aligned, every row leaves by the 8-byte path."""
    key = (name, "nv", nv)
    if key not in ls._built:
        ls._built[key] = problem_mod.resample_frequency(problem_of(name, ase_small, seed_small), nv)
    p = ls._built[key]
    assert p.beam.nv == nv and nv % 2 == 1
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, None)
    assert blocks[0]["Iv"].shape == (len(rays), nv)
    gate_blocks(blocks, oracle_blocks(oracle, p, rays, key), f"length spectra / {name}, K = {nv}", tight=name.startswith("seeded"))


@pytest.mark.parametrize("name", ["seeded forward", "emission backward"])
def test_a_strided_device_grid(hip, oracle, ase_small, seed_small, name):
    p = problem_of(name, ase_small, seed_small)
    ids = np.arange(3, p.n_rays_total, 7, dtype=np.int64)
    rays = p.build_rays(ids)
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, None, first=3, stride=7)
    assert info["stats"]["n_rays"] == len(rays) and len(rays) % 64 != 0
    gate_blocks(blocks, oracle_blocks(oracle, p, rays, (name, "strided")), f"length spectra / {name}, grid first 3 stride 7", tight=name.startswith("seeded"))


# ---------------------------------------------------------------------------------------------- 5. the sums against the scan plans' records
@pytest.mark.parametrize("name", PROBLEMS)
def test_the_sums_of_a_block_are_E_v_of_the_scan_record(hip, ase_small, seed_small, name):
    """E_v of record n (RayTraceImageCPU.cpp:59) is scale times the sum of Iv over the rays that deposit into a pixel: the
    same rows summed in another order, so the two agree within reordering_tol."""
    p = problem_of(name, ase_small, seed_small)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks, _ = run_lspec(plan, None)
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_step()
        (plan.enable_length_scan() if p.method == 2 else plan.enable_suffix_scan()).run()
        recs = plan.fetch_length_steps()
    for blk, rec in zip(blocks, recs):
        assert blk["n"] == rec["n"] and rec["failure_code"] == 0 and not blk["err"].any()
        ix, iy, _, _ = deposit_cells(sub(p, blk["n"]), rays, blk["ray2"])
        dep = (ix >= 0) & (iy >= 0)
        E_v = p.scale * blk["Iv"][dep].sum(axis=0)
        n_dep = int(dep.sum())
        assert_elements(E_v, rec["E_v"], np.array([n_dep]), float(reordering_tol(n_dep, p.beam.nv)),
                        f"length spectra / {name} / n = {blk['n']}: sums over the rays against E_v of the scan record")
        assert rec["E_v"].any()


# ---------------------------------------------------------------------------------------------- 6. mode hygiene
def test_refusals(hip, ase_small, seed_small):
    lib = hip.HipLibrary.get().lib
    ARG = cabi.RT_ERR_ARG

    def refused(rc, *words):
        text = lib.rt_hip_last_error()
        assert rc == ARG and all(w in text for w in words), (rc, text)

    six = sx.emission_backward(ase_small)
    fwd = ls.seeded_forward(seed_small)
    with hip.Plan(problem_mod.suffix_lengths(six, 2)) as plan:                  # N = 2
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"rt_hip_plan_enable_length_spectra", b"N < 3")
        assert lib.rt_hip_plan_enable_length_spectra(plan._h, 0) == 0           # (switching off what is off)
    refused(lib.rt_hip_plan_enable_length_spectra(None, 1), b"NULL plan")
    with hip.Plan(six) as plan:                                                 # each mode that is on refuses the switch, with its text
        plan.set_ray_grid()
        plan.enable_step()
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"step mode")
        plan.enable_suffix_scan()
        plan.enable_step(False)
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"suffix scan")
        plan.enable_suffix_scan(False)
        plan.enable_spectra()
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"spectra mode")
        plan.enable_spectra(False).enable_path()
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"path tracer")
        plan.enable_path(False)
        import ase_seeds as A
        sd = A.seeds_of(six)[0]
        plan.set_ase_seeds([sd])
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"ASE seeds")
        plan.set_ase_seeds([])
        # ... and while length spectra are on, each of those switches and installers is refused
        plan.enable_length_spectra()
        for call, word in ((plan.enable_step, "length spectra"), (plan.enable_spectra, "length spectra"), (plan.enable_path, "length spectra"),
                           (plan.enable_suffix_scan, "length spectra"), (lambda: plan.set_ase_seeds([sd]), "length spectra")):
            with pytest.raises(hip.RayTraceError, match=word):
                call()
        refused(lib.rt_hip_plan_set_suffix_ase_seeds(plan._h, 0, None, None), b"length spectra")    # (the installers of a scan's seeds as well)
        refused(lib.rt_hip_plan_set_scan_ase_seeds(plan._h, 0, None, None), b"length spectra")
        refused(lib.rt_hip_plan_enable_length_scan(plan._h, 1), b"length spectra")
        import torch
        buf = torch.zeros(six.beam.na * six.beam.nb + 64, dtype=torch.float64, device="cuda")
        with pytest.raises(hip.RayTraceError, match="no image buffers"):
            plan.run(iang_ptr=buf.data_ptr())
        plan.set_step_one_launch(True).run()                                    # (accepted; the run keeps two kernels)
        assert plan.last_fused() is False
        for n in (1, 7, 0, -1):
            refused(lib.rt_hip_plan_fetch_length_spectra(plan._h, n, None, None, None), b"n must be 2 .. N")
            refused(lib.rt_hip_plan_length_spectra_ptrs(plan._h, n, None, None, None), b"n must be 2 .. N")
        for n in range(2, 7):
            assert lib.rt_hip_plan_fetch_length_spectra(plan._h, n, None, None, None) == 0      # any pointer may be NULL
        refused(lib.rt_hip_plan_fetch_spectra(plan._h, None, None, None), b"not a spectra run")
        assert plan.spectra_ptr() == 0
        b = six.beam
        image = np.empty(b.nx * b.ny * b.nv)
        refused(lib.rt_hip_plan_fetch(plan._h, cabi._dp(image), None, None, None, 0, None, None), b"length-spectra run")
        plan.enable_length_spectra(False)
        refused(lib.rt_hip_plan_fetch_length_spectra(plan._h, 2, None, None, None), b"not a length-spectra run")
    with hip.Plan(fwd) as plan:                                                 # a seeded forward plan: seed set and length scan
        plan.set_ray_grid().set_seeds([fwd.seed])
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"seed set")
        plan.set_seeds([]).enable_length_scan()
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"length scan")
        plan.enable_length_scan(False).enable_length_spectra()
        for call in (lambda: plan.set_seeds([fwd.seed]), lambda: plan.set_scan_seeds([fwd.seed]), plan.enable_length_scan):
            with pytest.raises(hip.RayTraceError, match="length spectra"):
                call()
        refused(lib.rt_hip_plan_fetch_length_spectra(plan._h, 2, None, None, None), b"not a length-spectra run")       # has not run
    with hip.Plan(ls.scan_problem(ase_small, cabi.RT_N_SCAN_MAX + 2, scale_g0=False)) as plan:
        refused(lib.rt_hip_plan_enable_length_spectra(plan._h, 1), b"RT_N_SCAN_MAX")


@pytest.mark.parametrize("name", ["seeded forward", "emission backward"])
def test_switching_off_restores_the_plan(hip, oracle, ase_small, seed_small, name):
    """A plan that has been in length-spectra mode and left it runs as a fresh plan does: the same march instance, the same
    march records and exit rays bit for bit (the probe), the same spectra bit for bit; image and I_ang -- sums by atomics,
    whose order differs between two runs of ONE plan as well -- within reordering_tol."""
    p = problem_of(name, ase_small, seed_small)
    with hip.Plan(p) as fresh:
        fresh.set_ray_grid().enable_probe().run()
        want, want_probe, inst = fresh.fetch(), fresh.fetch_probe(), fresh.last_march_instance()
        want_spec = fresh.enable_spectra().run().fetch_spectra()
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_probe().enable_length_spectra().run()
        assert len(plan.fetch_length_spectra()) == 5
        plan.enable_length_spectra(False).run()
        got, got_probe = plan.fetch(), plan.fetch_probe()
        assert plan.last_march_instance() == inst and not inst & (8 << 1)
        got_spec = plan.enable_spectra().run().fetch_spectra()
    assert got["failure_code"] == want["failure_code"] == 0 and got["image"] is not None
    for key in ("gvl", "evl", "ivl", "ray2", "flags", "steps"):
        assert want_probe[key].tobytes() == got_probe[key].tobytes(), key
    for key in ("Iv", "ray2", "err"):
        assert want_spec[key].tobytes() == got_spec[key].tobytes(), key
    rays = p.build_rays()
    counts = contribution_counts(p, rays, want_probe["ray2"], want_spec["err"])
    gate_outputs(got, want, p, counts, "reordering", f"length spectra switched off / {name}: image mode against a fresh plan")


@pytest.mark.parametrize("name", ["seeded forward", "emission backward"])
def test_update_gain_keeps_the_mode(hip, oracle, ase_small, seed_small, name):
    p = problem_of(name, ase_small, seed_small)
    key = (name, "tables_b")
    if key not in ls._built:
        ls._built[key] = tv.tables_b(p)
    pb = ls._built[key]
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks_a, _ = run_lspec(plan, None)
        plan.update_gain(pb.gain).run()
        info = plan.fetch()
        blocks_b = plan.fetch_length_spectra()
    assert not np.array_equal(blocks_a[0]["Iv"], blocks_b[0]["Iv"]) and info["failure_code"] == 0
    gate_blocks(blocks_b, oracle_blocks(oracle, pb, rays, key, fresh=True), f"length spectra / {name} after update_gain (tables B)",
                tight=name.startswith("seeded"))


@pytest.mark.parametrize("name", PROBLEMS)
def test_the_probe_is_that_of_the_whole_run(hip, ase_small, seed_small, name):
    p = problem_of(name, ase_small, seed_small)
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_probe().enable_spectra().run()
        plain = plan.fetch_probe()
        plan.enable_spectra(False).enable_length_spectra().run()
        scan = plan.fetch_probe()
        last = plan.fetch_length_spectra()[-1]
    for key in ("gvl", "evl", "ivl", "ray2", "flags", "steps"):
        assert plain[key].tobytes() == scan[key].tobytes(), key
    assert (plain["flags"] & 1).any() and plain["steps"].any()
    assert last["ray2"].tobytes() == scan["ray2"].tobytes()          # block N is the whole run


@pytest.mark.parametrize("name", ["seeded forward", "emission backward"])
def test_calc_rays_lengths_equals_the_plans_rows(hip, ase_small, seed_small, name):
    p = problem_of(name, ase_small, seed_small)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks, info = run_lspec(plan, rays)
    out = hip.calc_rays_lengths(p, rays)
    assert out["failure_code"] == info["failure_code"] == 0 and len(out["lengths"]) == 5
    assert out["stats"]["cell_steps"] == info["stats"]["cell_steps"] and out["stats"]["n_rays"] == len(rays)
    for a, b in zip(out["lengths"], blocks):
        assert a["n"] == b["n"]
        for key in ("Iv", "ray2", "err"):
            assert a[key].tobytes() == b[key].tobytes(), (a["n"], key)
    # an [n][4] float64 array is taken as calc_rays takes it
    again = hip.calc_rays_lengths(p, cabi.rays_to_array(rays[:70]).astype(np.float64), exact=True)
    assert again["lengths"][0]["Iv"].shape == (70, p.beam.nv)
