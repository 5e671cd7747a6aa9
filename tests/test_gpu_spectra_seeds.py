"""Spectra seeds on the GPU (rt_hip_plan_set_spectra_seeds; rt_spec_seeds_kernel, rt_spec_scan_seeds_kernel): RayTrace::calc_ray
for every ray under two seed beams from ONE march -- in spectra mode and, at every plasma length n = 2 .. N, in length spectra.

Inputs (tests/spectra_seeds.py): length_scan.seeded_forward and suffix_scan.seeded_backward of seed_small, 1 350 rays (21 tiles and
a ragged one of 6), K = 82 (five groups of 16 and a left-over of two); seed 0 the problem's own, seed 1 seed_scan.primed of the
`narrow` profile (another support, f[4] reversed in k, another f0).  tests/test_spectra_seeds_host.py asserts the census these
tests rest on: under each seed and at each n at least 40 rows are clean and non-zero, and the seeds light different rays.

Gates.  Against the oracle's probe of the (sub-)problem created with seed s: err equal ray by ray, ray2 bit for bit where
err != -1, rows that are zero on the CPU zero here, Iv per ray inside the tight tier (TIGHT_TIER = 1e-11, gain-only mode), no
clean row left out.  Against the single-seed spectra (length-spectra) plan created with seed s: EQUAL bit for bit -- the values
are the same doubles and nothing is summed.  The measured figures (expected: 0 differing elements) are printed before every
assertion; with SPECTRA_PARITY_FILE set they are appended to that file (profiles/spectra_seeds_parity.txt)."""
import importlib

import numpy as np
import pytest

import length_scan as ls
import method_pairs as mp
import seed_profiles as sp
import seed_scan as sc
import spectra_seeds as S
from element_gate import TIGHT_TIER
from test_gpu_spectra import check_against, note, ray2_bits_equal, row_figures

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

METHODS = [1, 2]
_refs = {}


# ---------------------------------------------------------------------------------------------- helpers
def spectra_refs(oracle, p, seeds, rays, key):
    """Per seed the oracle's probe of p created with that seed; once per key, left unchanged."""
    if key not in _refs:
        _refs[key] = [S.probe_of(oracle, p, sd, rays) for sd in seeds]
    return _refs[key]


def length_refs(oracle, p, seeds, rays, key):
    """Per seed {n: the oracle's probe of the sub-problem of n lengths created with that seed}."""
    if key not in _refs:
        _refs[key] = [{n: S.probe_of(oracle, S.sub(p, n), sd, rays) for n in range(2, p.N + 1)} for sd in seeds]
    return _refs[key]


def run_spec(plan, seeds, rays, **grid):
    (plan.set_ray_grid(**grid) if rays is None else plan.set_rays(rays))
    plan.enable_spectra().set_spectra_seeds(seeds).run()
    info = plan.fetch()
    return plan.fetch_seed_spectra(), info


def run_lspec(plan, seeds, rays, **grid):
    (plan.set_ray_grid(**grid) if rays is None else plan.set_rays(rays))
    plan.enable_length_spectra().set_spectra_seeds(seeds).run()
    info = plan.fetch()
    return plan.fetch_seed_length_spectra(), info


def gate_rows(blk, ref, label):
    """One block of rows against the oracle: check_against, the tight tier, no clean row left out.  Returns the per-ray rel-L2."""
    rows, nzero = check_against(blk, ref, label)
    assert rows + nzero == int((ref["err"] == 0).sum()), label      # no row with err = 0 in the oracle is left out
    ok = ref["err"] == 0
    l2 = row_figures(blk["Iv"][ok], ref["Iv"][ok])[0]
    assert l2 < TIGHT_TIER, (label, l2)
    return l2, rows


def gate_seeds(blocks, refs, label):
    assert len(blocks) == len(refs)
    worst = 0.0
    for s, (blk, ref) in enumerate(zip(blocks, refs)):
        l2, rows = gate_rows(blk, ref, f"{label} / seed {s}")
        worst = max(worst, l2)
    note(f"{label}: worst per-ray rel-L2 over the seeds {worst:.3e} (tight tier 1e-11)")


def gate_seed_lengths(curves, refs, label):
    assert len(curves) == len(refs)
    worst = 0.0
    for s, (curve, ref) in enumerate(zip(curves, refs)):
        assert [b["n"] for b in curve] == sorted(ref)
        for blk in curve:
            worst = max(worst, gate_rows(blk, ref[blk["n"]], f"{label} / seed {s} / n = {blk['n']}")[0])
    note(f"{label}: worst per-ray rel-L2 over all (seed, n) {worst:.3e} (tight tier 1e-11)")


def bits_differ(a, b, label):
    """Elements of two spectra that are not the same double (expected: 0), noted before the caller asserts."""
    diff = a["Iv"].view(np.uint64) != b["Iv"].view(np.uint64)
    nz = b["Iv"] != 0
    both = nz & np.isfinite(b["Iv"]) & np.isfinite(a["Iv"])
    rel = float((np.abs(a["Iv"] - b["Iv"])[both] / np.abs(b["Iv"])[both]).max()) if both.any() else 0.0
    note(f"{label}: differing elements {int(diff.sum())} of {diff.size} in {int(diff.any(axis=1).sum())} rows, max rel diff {rel:.3e}")
    return int(diff.sum())


def same_rows(a, b, label):
    assert np.array_equal(a["err"], b["err"]), label
    assert ray2_bits_equal(a["ray2"], b["ray2"], b["err"] != -1), label
    assert bits_differ(a, b, label) == 0, label


def single_spectra(hip, p, seed, rays, **grid):
    with hip.Plan(sc.with_seed(p, seed, "created with this seed")) as plan:
        (plan.set_ray_grid(**grid) if rays is None else plan.set_rays(rays))
        return plan.enable_spectra().run().fetch_spectra()


def single_length_spectra(hip, p, seed, rays, **grid):
    with hip.Plan(sc.with_seed(p, seed, "created with this seed")) as plan:
        (plan.set_ray_grid(**grid) if rays is None else plan.set_rays(rays))
        plan.enable_length_spectra().run()
        info = plan.fetch()
        return plan.fetch_length_spectra(), info


def check_report(info, err_blocks, rays, label):
    """failure_code is the OR of the codes over every block of err; every ray failing in any block is reported once (more than
    RT_N_FAILED_MAX: the first of them in list order)."""
    code, failing = 0, np.zeros(len(rays), bool)
    for err in err_blocks:
        code |= S.code_of(err)
        failing |= err != 0
    want = [tuple(r) for r in rays[failing].tolist()]
    got = [tuple(r) for r in info["failed_rays"].tolist()]
    print(f"{label}: failure_code {info['failure_code']} (oracle {code}), failing rays {len(want)}, reported {len(got)}")
    assert info["failure_code"] == code, label
    assert len(got) == len(set(got)), label                                                     # each once
    if len(want) > cabi.RT_N_FAILED_MAX:
        assert got == want[:cabi.RT_N_FAILED_MAX], label
    else:
        assert sorted(got) == sorted(want), label


# ---------------------------------------------------------------------------------------------- 1. spectra mode against the oracle
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("N", [3, 6])
@pytest.mark.parametrize("method", METHODS)
def test_spectra_mode_against_the_oracle(hip, oracle, seed_small, method, N, mode):
    """N = 3 takes rt_spec_seeds_kernel<6>, N = 6 the generic instance."""
    p = S.problem_of(seed_small, method, N)
    seeds = S.seeds_of(p, seed_small)
    rays = p.build_rays()
    refs = spectra_refs(oracle, p, seeds, rays, ("spec", method, N))
    with hip.Plan(p) as plan:
        blocks, info = run_spec(plan, seeds, None if mode == "grid" else rays)
        assert info["stats"]["n_rays"] == len(rays) and plan.last_fused() is False and info["image"] is None
        assert not plan.last_march_instance() & (8 << 1)                      # the march of spectra mode, not the scan instance
    assert len(blocks) == 2 and info["failure_code"] == 0
    gate_seeds(blocks, refs, f"spectra seeds / method {method}, N = {N}, ray {mode}")
    assert blocks[0]["ray2"].tobytes() == blocks[1]["ray2"].tobytes()
    assert blocks[0]["Iv"].any() and blocks[1]["Iv"].any() and not np.array_equal(blocks[0]["Iv"], blocks[1]["Iv"])
    assert not np.array_equal(blocks[0]["Iv"].any(axis=1), blocks[1]["Iv"].any(axis=1))         # the seeds light different rays


# ---------------------------------------------------------------------------------------------- 2. bit-equal to the single-seed plans
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("N", [3, 6])
@pytest.mark.parametrize("method", METHODS)
def test_spectra_block_equals_the_plan_created_with_that_seed(hip, seed_small, method, N, mode):
    p = S.problem_of(seed_small, method, N)
    seeds = S.seeds_of(p, seed_small)
    rays = None if mode == "grid" else p.build_rays()
    with hip.Plan(p) as plan:
        blocks, _ = run_spec(plan, seeds, rays)
    for s, sd in enumerate(seeds):
        same_rows(blocks[s], single_spectra(hip, p, sd, rays),
                  f"spectra seeds / method {method}, N = {N}, ray {mode} / seed {s} against the spectra plan created with it")


@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("method", METHODS)
def test_length_spectra_block_equals_the_plan_created_with_that_seed(hip, seed_small, method, mode):
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    rays = None if mode == "grid" else p.build_rays()
    with hip.Plan(p) as plan:
        curves, _ = run_lspec(plan, seeds, rays)
    for s, sd in enumerate(seeds):
        one, _ = single_length_spectra(hip, p, sd, rays)
        assert len(curves[s]) == len(one) == 5
        for a, b in zip(curves[s], one):
            assert a["n"] == b["n"]
            same_rows(a, b, f"length spectra seeds / method {method}, ray {mode} / seed {s}, n = {a['n']} against the length-spectra plan created with it")
            assert a["ray2"].tobytes() == b["ray2"].tobytes()                                    # ray2 [L][n_rays] is the single-seed plan's


# ---------------------------------------------------------------------------------------------- 3. length spectra against the oracle
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("method", METHODS)
def test_length_spectra_against_the_oracle(hip, oracle, seed_small, method, mode):
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    rays = p.build_rays()
    refs = length_refs(oracle, p, seeds, rays, ("lspec", method))
    with hip.Plan(p) as plan:
        curves, info = run_lspec(plan, seeds, None if mode == "grid" else rays)
        assert plan.last_march_instance() & (8 << 1) and plan.last_fused() is False             # the scan instance of the march
        full = oracle.image_loop(p, rays)
        assert info["stats"]["cell_steps"] == full["counters"]["cell_steps"]                    # the march of all N lengths, once
        views = plan.seed_length_spectra_tensors()
        L, K, nr = p.N - 1, p.beam.nv, len(rays)
        assert tuple(views["Iv"].shape) == (2, L, nr, K) and tuple(views["err"].shape) == (2, L, nr) and tuple(views["ray2"].shape) == (L, nr, 4)
        assert plan.seed_length_spectra_ptrs(0, 2) == plan.length_spectra_ptrs(2)               # block 0 is seed 0
        assert plan.seed_length_spectra_ptrs(1, 2)[0] == plan.seed_length_spectra_ptrs(0, 2)[0] + 8 * L * nr * K      # seed-major
        assert plan.seed_length_spectra_ptrs(1, 3)[1] == plan.length_spectra_ptrs(3)[1]         # one ray2 for every seed
        iv, er, r2 = views["Iv"].cpu().numpy(), views["err"].cpu().numpy(), views["ray2"].cpu().numpy()
        plain = plan.fetch_length_spectra()                                                     # the plain fetcher serves seed 0
    assert info["failure_code"] == 0 and len(curves) == 2 and all(len(c) == 5 for c in curves)
    gate_seed_lengths(curves, refs, f"length spectra seeds / method {method}, ray {mode}")
    for s in range(2):
        for j, blk in enumerate(curves[s]):
            assert np.array_equal(iv[s, j], blk["Iv"], equal_nan=True) and np.array_equal(er[s, j], blk["err"])
            assert np.array_equal(r2[j].view(np.uint32), cabi.rays_to_array(blk["ray2"]).astype(np.float32).view(np.uint32))
    for a, b in zip(plain, curves[0]):
        for key in ("Iv", "ray2", "err"):
            assert a[key].tobytes() == b[key].tobytes(), (a["n"], key)
    for n in range(2, 7):
        a, b = curves[0][n - 2]["Iv"].any(axis=1), curves[1][n - 2]["Iv"].any(axis=1)
        assert a.sum() >= 40 and b.sum() >= 40 and not np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 4. codes per seed and length
@pytest.mark.parametrize("method", METHODS)
def test_codes_per_seed_in_spectra_mode(hip, oracle, seed_small, method):
    p, seeds = S.failing(S.problem_of(seed_small, method), seed_small)
    rays = p.build_rays()
    refs = spectra_refs(oracle, p, seeds, rays, ("spec failing", method))
    codes = [S.code_of(r["err"]) for r in refs]
    assert codes == [S.WANT_CODES[method][0][-1], S.WANT_CODES[method][1][-1]] and codes[0] != codes[1]
    for mode_rays in (None, rays):
        with hip.Plan(p) as plan:
            blocks, info = run_spec(plan, seeds, mode_rays)
        for s in range(2):
            check_against(blocks[s], refs[s], f"spectra seeds, failing variant / method {method} / seed {s}")
            assert S.code_of(blocks[s]["err"]) == codes[s]
        check_report(info, [r["err"] for r in refs], rays, f"spectra seeds, failing variant / method {method}")


@pytest.mark.parametrize("method", METHODS)
def test_codes_per_seed_and_length(hip, oracle, seed_small, method):
    p, seeds = S.failing(S.problem_of(seed_small, method), seed_small)
    rays = p.build_rays()
    refs = length_refs(oracle, p, seeds, rays, ("lspec failing", method))
    want = [[S.code_of(refs[s][n]["err"]) for n in range(2, 7)] for s in range(2)]
    assert want == S.WANT_CODES[method]
    for mode_rays in (None, rays):
        with hip.Plan(p) as plan:
            curves, info = run_lspec(plan, seeds, mode_rays)
        for s in range(2):
            for blk in curves[s]:
                check_against(blk, refs[s][blk["n"]], f"length spectra seeds, failing variant / method {method} / seed {s}, n = {blk['n']}")
            assert [S.code_of(b["err"]) for b in curves[s]] == want[s]
        check_report(info, [refs[s][n]["err"] for s in range(2) for n in refs[s]], rays, f"length spectra seeds, failing variant / method {method}")


@pytest.mark.parametrize("lengths", [False, True])
@pytest.mark.parametrize("method", METHODS)
def test_a_steep_ray_fails_under_every_seed(hip, oracle, seed_small, method, lengths):
    """One ray launched almost perpendicular to z (s.z^2 < 0.01, Helper.h:515): error -1 under every seed (and n), zeros, reported once."""
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    bad = p.build_rays().copy()
    bad["a"][7] = 1500.0
    with hip.Plan(p) as plan:
        out, info = (run_lspec if lengths else run_spec)(plan, seeds, bad)
    for s, sd in enumerate(seeds):
        for blk in (out[s] if lengths else [out[s]]):
            ref = S.probe_of(oracle, S.sub(p, blk["n"]) if lengths else p, sd, bad)
            assert ref["err"][7] == -1 and blk["err"][7] == -1 and not blk["Iv"][7].any()
            assert all(blk["ray2"][k][7] == 0 for k in "xyab")
            check_against(blk, ref, f"spectra seeds, a steep ray / method {method} / seed {s}")
    assert info["failure_code"] == 1 << 1 and len(info["failed_rays"]) == 1 and info["failed_rays"][0] == bad[7]


# ---------------------------------------------------------------------------------------------- 5. shapes where the stores can go wrong
def both_modes_against_the_oracle(hip, oracle, p, seeds, rays, key, label, **grid):
    refs = spectra_refs(oracle, p, seeds, rays, ("spec",) + key)
    lrefs = length_refs(oracle, p, seeds, rays, ("lspec",) + key)
    with hip.Plan(p) as plan:
        blocks, info = run_spec(plan, seeds, None if grid else rays, **grid)
        assert info["stats"]["n_rays"] == len(rays)
        gate_seeds(blocks, refs, f"spectra seeds / {label}")
        plan.enable_spectra(False)                                                              # (drops the seeds)
        curves, info = run_lspec(plan, seeds, None if grid else rays, **grid)
        assert info["stats"]["n_rays"] == len(rays)
        gate_seed_lengths(curves, lrefs, f"length spectra seeds / {label}")
    return blocks, curves


@pytest.mark.parametrize("n_rays", [1, 64])
@pytest.mark.parametrize("method", METHODS)
def test_one_ray_and_one_full_tile(hip, oracle, seed_small, method, n_rays):
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    rays = p.build_rays()[611:611 + n_rays].copy()
    both_modes_against_the_oracle(hip, oracle, p, seeds, rays, (method, "rays", n_rays), f"method {method}, {n_rays} ray(s)")


@pytest.mark.parametrize("method", METHODS)
def test_ten_lengths_ragged_tile(hip, oracle, seed_small, method):
    """N = 10 on 450 rays: nine blocks are five backward walks of two suffixes, the last tile holds two rays."""
    key = ("spectra seeds e2e10", method)
    if key not in ls._built:
        base = mp.seed_backward(seed_small) if method == 1 else seed_small
        ls._built[key] = ls.scan_problem(sp.e2e_problem(base, "limiter"), 10)
    p = ls._built[key]
    assert p.n_rays_total == 450 and p.N == 10 and p.method == method
    seeds = (p.seed, sc.primed(sp.e2e_problem(seed_small, "narrow").seed))
    rays = p.build_rays()
    for grid in (dict(), dict(first=0, stride=1)):
        _, curves = both_modes_against_the_oracle(hip, oracle, p, seeds, rays, (method, "N10"), f"method {method}, N = 10, 450 rays, {'grid' if grid else 'list'}", **grid)
        assert all(len(c) == 9 for c in curves)


@pytest.mark.parametrize("method", METHODS)
def test_an_odd_number_of_frequencies(hip, oracle, seed_small, method):
    """An odd K (the construction of tests/test_gpu_length_spectra.py): no 16-byte store is aligned, every row leaves by the 8-byte path."""
    key = ("spectra seeds nv", method, 81)
    if key not in ls._built:
        ls._built[key] = problem_mod.resample_frequency(S.problem_of(seed_small, method), 81)
    p = ls._built[key]
    assert p.beam.nv == 81
    seeds = (p.seed, sc.primed(p.seed))                                  # (seed 1 on the resampled frequency axis: f[4] reversed, f0 x 0.37)
    rays = p.build_rays()
    blocks, curves = both_modes_against_the_oracle(hip, oracle, p, seeds, rays, (method, "K81"), f"method {method}, K = 81", first=0, stride=1)
    assert blocks[0]["Iv"].shape == (len(rays), 81) and curves[1][0]["Iv"].shape == (len(rays), 81)


@pytest.mark.parametrize("method", METHODS)
def test_one_seed(hip, oracle, seed_small, method):
    """n_seed = 1, and that one not the creation seed: the rows are those of a plan created with it."""
    p = S.problem_of(seed_small, method)
    seed1 = S.seeds_of(p, seed_small)[1]
    rays = p.build_rays()
    blocks, curves = both_modes_against_the_oracle(hip, oracle, p, (seed1,), rays, (method, "one seed"), f"method {method}, n_seed = 1")
    assert len(blocks) == 1 and len(curves) == 1
    same_rows(blocks[0], single_spectra(hip, p, seed1, rays), f"spectra seeds / method {method}, n_seed = 1 against the plan created with it")


@pytest.mark.parametrize("method", METHODS)
def test_a_strided_device_grid(hip, oracle, seed_small, method):
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    rays = p.build_rays(np.arange(3, p.n_rays_total, 7, dtype=np.int64))
    assert len(rays) % 64 != 0
    both_modes_against_the_oracle(hip, oracle, p, seeds, rays, (method, "strided"), f"method {method}, grid first 3 stride 7", first=3, stride=7)


# ---------------------------------------------------------------------------------------------- 6. state
@pytest.mark.parametrize("method", METHODS)
def test_seed_0_is_served_by_the_plain_fetchers_and_the_tensors_view_the_rows(hip, seed_small, method):
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    nr, K = p.n_rays_total, p.beam.nv
    with hip.Plan(p) as plan:
        blocks, _ = run_spec(plan, seeds, None)
        plain = plan.fetch_spectra()
        for key in ("Iv", "ray2", "err"):
            assert plain[key].tobytes() == blocks[0][key].tobytes(), key
        assert plan.spectra_ptr() == plan.seed_spectra_ptrs(0)[0]
        assert plan.seed_spectra_ptrs(1)[0] == plan.spectra_ptr() + 8 * nr * K                  # seed-major
        assert plan.seed_spectra_ptrs(1)[1] == plan.seed_spectra_ptrs(0)[1]                     # one ray2
        assert plan.seed_spectra_ptrs(1)[2] == plan.seed_spectra_ptrs(0)[2] + 4 * nr
        views = plan.seed_spectra_tensors()
        assert tuple(views["Iv"].shape) == (2, nr, K) and tuple(views["err"].shape) == (2, nr) and tuple(views["ray2"].shape) == (nr, 4)
        assert views["Iv"].data_ptr() == plan.spectra_ptr()
        iv, er, r2 = views["Iv"].cpu().numpy(), views["err"].cpu().numpy(), views["ray2"].cpu().numpy()
        for s in range(2):
            assert np.array_equal(iv[s], blocks[s]["Iv"], equal_nan=True) and np.array_equal(er[s], blocks[s]["err"])
        assert np.array_equal(r2.view(np.uint32), cabi.rays_to_array(blocks[0]["ray2"]).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("method", METHODS)
def test_removing_the_seeds_restores_the_plan_of_the_creation_seed(hip, seed_small, method):
    """set_spectra_seeds([]) leaves the plain modes bit for bit (no atomics on data); switching a mode off drops the seeds;
    a rejected call leaves them."""
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    lib = hip.HipLibrary.get().lib
    with hip.Plan(p) as fresh:
        want = fresh.set_ray_grid().enable_spectra().run().fetch_spectra()
        fresh.enable_spectra(False).enable_length_spectra().run()
        want_l = fresh.fetch_length_spectra()
    with hip.Plan(p) as plan:
        with_seeds, _ = run_spec(plan, seeds, None)
        # a rejected call leaves the installed seeds
        arr = (cabi.RtSeed * 3)()
        assert lib.rt_hip_plan_set_spectra_seeds(plan._h, 3, arr) == cabi.RT_ERR_ARG and b"more than RT_N_SEED_MAX" in lib.rt_hip_last_error()
        assert lib.rt_hip_plan_set_spectra_seeds(plan._h, 1, arr) == cabi.RT_ERR_ARG and b"incomplete seed table" in lib.rt_hip_last_error()
        again = plan.run().fetch_seed_spectra()
        for s in range(2):
            assert again[s]["Iv"].tobytes() == with_seeds[s]["Iv"].tobytes() and again[s]["err"].tobytes() == with_seeds[s]["err"].tobytes()
        # removing them
        got = plan.set_spectra_seeds([]).run().fetch_spectra()
        for key in ("Iv", "ray2", "err"):
            assert want[key].tobytes() == got[key].tobytes(), key
        with pytest.raises(hip.RayTraceError, match="spectra seeds"):
            plan.seed_spectra_ptrs(0)
        # enable_spectra(False) drops the seeds: length spectra then run with the creation seed alone
        plan.set_spectra_seeds(seeds).enable_spectra(False)
        assert plan._n_spec_seed == 0
        got_l = plan.enable_length_spectra().run().fetch_length_spectra()
        for a, b in zip(want_l, got_l):
            for key in ("Iv", "ray2", "err"):
                assert a[key].tobytes() == b[key].tobytes(), (a["n"], key)
        with pytest.raises(hip.RayTraceError, match="no spectra seeds"):
            plan.seed_length_spectra_ptrs(0, 2)
        # ... and so does enable_length_spectra(False); set_spectra_seeds([]) in length spectra restores them as well
        curves = plan.set_spectra_seeds(seeds).run().fetch_seed_length_spectra()
        assert len(curves) == 2 and curves[1][0]["Iv"].any()
        got_l = plan.set_spectra_seeds([]).run().fetch_length_spectra()
        for a, b in zip(want_l, got_l):
            assert a["Iv"].tobytes() == b["Iv"].tobytes() and a["err"].tobytes() == b["err"].tobytes()
        plan.set_spectra_seeds(seeds).enable_length_spectra(False)
        got = plan.enable_spectra().run().fetch_spectra()
        assert want["Iv"].tobytes() == got["Iv"].tobytes() and plan.fetch_seed_spectra() == []


@pytest.mark.parametrize("method", METHODS)
def test_update_gain_keeps_the_seeds(hip, oracle, seed_small, method):
    import table_variants as tv

    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    key = ("spectra seeds tables_b", method)
    if key not in ls._built:
        ls._built[key] = tv.tables_b(p)
    pb = ls._built[key]
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        before, _ = run_spec(plan, seeds, None)
        plan.update_gain(pb.gain).run()
        info = plan.fetch()
        after = plan.fetch_seed_spectra()
        assert len(after) == 2 and info["failure_code"] == 0 and not np.array_equal(before[1]["Iv"], after[1]["Iv"])
        gate_seeds(after, spectra_refs(oracle, pb, seeds, rays, ("spec tables_b", method)), f"spectra seeds after update_gain (tables B) / method {method}")
        plan.enable_spectra(False).update_gain(p.gain)
        curves, _ = run_lspec(plan, seeds, None)
        plan.update_gain(pb.gain).run()
        lafter = plan.fetch_seed_length_spectra()
        assert len(lafter) == 2 and not np.array_equal(curves[1][-1]["Iv"], lafter[1][-1]["Iv"])
        gate_seed_lengths(lafter, length_refs(oracle, pb, seeds, rays, ("lspec tables_b", method)),
                          f"length spectra seeds after update_gain (tables B) / method {method}")


def test_refusals(hip, ase_small, seed_small):
    lib = hip.HipLibrary.get().lib
    ARG = cabi.RT_ERR_ARG

    def refused(rc, *words):
        text = lib.rt_hip_last_error()
        assert rc == ARG and all(w in text for w in words), (rc, text)

    p = S.problem_of(seed_small, 2)
    seeds, arr, _keep = hip._seed_array(S.seeds_of(p, seed_small), "test", "test")
    refused(lib.rt_hip_plan_set_spectra_seeds(None, 1, arr), b"rt_hip_plan_set_spectra_seeds", b"NULL plan")
    with hip.Plan(ls.emission_forward(ase_small)) as plan:                                     # an emission plan
        plan.set_ray_grid().enable_spectra()
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 1, arr), b"created without a seed", b"ASE seeds are not built")
    with hip.Plan(p) as plan:
        plan.set_ray_grid()
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 2, arr), b"neither spectra mode nor length spectra")
        plan.enable_step()
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 2, arr), b"neither spectra mode nor length spectra")
        plan.enable_step(False).enable_spectra()
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 3, arr), b"more than RT_N_SEED_MAX")
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, -1, arr), b"n_seed must be 0 .. RT_N_SEED_MAX")
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 2, None), b"NULL seeds")
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 1, (cabi.RtSeed * 1)()), b"incomplete seed table")
        assert lib.rt_hip_plan_set_spectra_seeds(plan._h, 0, None) == 0                         # (removing what is not there)
        refused(lib.rt_hip_plan_fetch_seed_spectra(plan._h, 0, None, None, None), b"not a spectra run with spectra seeds")      # has not run
        plan.run()
        refused(lib.rt_hip_plan_fetch_seed_spectra(plan._h, 0, None, None, None), b"not a spectra run with spectra seeds")      # ran without seeds
        plan.set_spectra_seeds(seeds).run()
        for s in (-1, 2):
            refused(lib.rt_hip_plan_fetch_seed_spectra(plan._h, s, None, None, None), b"s must be 0 .. n_seed - 1")
            refused(lib.rt_hip_plan_seed_spectra_ptrs(plan._h, s, None, None, None), b"s must be 0 .. n_seed - 1")
        assert lib.rt_hip_plan_fetch_seed_spectra(plan._h, 1, None, None, None) == 0            # any pointer may be NULL
        refused(lib.rt_hip_plan_fetch_seed_length_spectra(plan._h, 0, 2, None, None, None), b"not a length-spectra run")
        # while the seeds are installed spectra mode is on: every switch and installer refuses as it always has
        for call, word in ((plan.enable_step, "spectra mode"), (plan.enable_path, "spectra mode"), (plan.enable_length_spectra, "spectra mode"),
                           (plan.enable_length_scan, "spectra mode"), (lambda: plan.set_seeds([p.seed]), "spectra mode")):
            with pytest.raises(hip.RayTraceError, match=word):
                call()
        assert lib.rt_hip_plan_set_seeds(plan._h, 0, None) == 0                                 # (no set to remove: the spectra seeds stay)
        assert len(plan.run().fetch_seed_spectra()) == 2
        plan.enable_spectra(False).enable_length_spectra().set_spectra_seeds(seeds).run()
        for n in (1, 7):
            refused(lib.rt_hip_plan_fetch_seed_length_spectra(plan._h, 0, n, None, None, None), b"n must be 2 .. N")
        refused(lib.rt_hip_plan_seed_length_spectra_ptrs(plan._h, 2, 2, None, None, None), b"s must be 0 .. n_seed - 1")
        refused(lib.rt_hip_plan_fetch_seed_spectra(plan._h, 0, None, None, None), b"not a spectra run with spectra seeds")
        for call in (lambda: plan.set_seeds([p.seed]), lambda: plan.set_scan_seeds([p.seed]), plan.enable_spectra, plan.enable_step):
            with pytest.raises(hip.RayTraceError, match="length spectra"):
                call()
        plan.set_spectra_seeds([]).run()
        refused(lib.rt_hip_plan_fetch_seed_length_spectra(plan._h, 0, 2, None, None, None), b"no spectra seeds")


@pytest.mark.parametrize("method", METHODS)
def test_the_one_call_forms_equal_the_plans_rows(hip, seed_small, method):
    p = S.problem_of(seed_small, method)
    seeds = S.seeds_of(p, seed_small)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks, info = run_spec(plan, seeds, rays)
        plan.enable_spectra(False)
        curves, linfo = run_lspec(plan, seeds, rays)
    out = hip.calc_rays_seeds(p, seeds, rays)
    assert out["failure_code"] == info["failure_code"] == 0 and len(out["seeds"]) == 2
    assert out["stats"]["cell_steps"] == info["stats"]["cell_steps"] and out["stats"]["n_rays"] == len(rays)
    for a, b in zip(out["seeds"], blocks):
        for key in ("Iv", "ray2", "err"):
            assert a[key].tobytes() == b[key].tobytes(), key
    lout = hip.calc_rays_seeds_lengths(p, seeds, rays)
    assert lout["failure_code"] == linfo["failure_code"] == 0 and [len(c) for c in lout["seeds"]] == [5, 5]
    for ca, cb in zip(lout["seeds"], curves):
        for a, b in zip(ca, cb):
            assert a["n"] == b["n"]
            for key in ("Iv", "ray2", "err"):
                assert a[key].tobytes() == b[key].tobytes(), (a["n"], key)
    # an [n][4] float64 array is taken as calc_rays takes it
    again = hip.calc_rays_seeds(p, seeds[1:], cabi.rays_to_array(rays[:70]).astype(np.float64))
    assert len(again["seeds"]) == 1 and again["seeds"][0]["Iv"].shape == (70, p.beam.nv)
