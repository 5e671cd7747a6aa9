"""Spectra mode with ASE seeds on the GPU (rt_hip_plan_set_spectra_ase_seeds; rt_spec_ase_seeds_kernel<6>, <0>):
RayTrace::calc_ray of an emission problem AND of the same problem under two seed beams, for every ray, from ONE march.

Inputs (tests/spectra_ase_seeds.py): ase_seeds.base(ase_small, method, N) -- 1 440 rays (22 tiles and a ragged one of 32), K = 52
(three groups of 16 and a left-over of 4), N = 3 (<6>) and N = 5 (<0>), as a ray list and as a ray grid; the seeds `wide` and
`narrow`.  tests/test_spectra_ase_seeds_host.py asserts the census these tests rest on.

Gates.  Against the oracle: block 0 is the probe of p -- DEFAULT_TIER (1e-5) per ray in the default emission mode, TIGHT_TIER
(1e-11) with exact emission; block 1 + s is the probe of ase_seeds.carry(p, seed_s) -- TIGHT_TIER; err equal ray by ray, ray2 bit
for bit where err != -1, rows that are zero on the CPU zero here, every row with err = 0 in the oracle compared.  Against the
plans the one plan replaces, as an EQUALITY: block 0 is bit for bit the plain spectra run of the same plan (default and exact
emission), block 1 + s bit for bit the spectra plan of carry(p, seed_s); 0 differing elements are asserted, the count is noted
first.  With SPECTRA_PARITY_FILE set the figures are appended to that file (profiles/spectra_ase_seeds_parity.txt)."""
import copy
import importlib

import numpy as np
import pytest

import ase_seeds as A
import method_pairs as mp
import spectra_ase_seeds as S
import table_variants as tv
import update_regimes as ur
from element_gate import DEFAULT_TIER, TIGHT_TIER
from test_gpu_spectra import check_against, note, row_figures

rt = importlib.import_module("raytrace-miniapp_amd")
cabi = rt.cabi
pytestmark = pytest.mark.gpu

METHODS = [1, 2]
_plain = {}


# ---------------------------------------------------------------------------------------------- helpers
def set_rays(plan, rays, **grid):
    return plan.set_ray_grid(**grid) if rays is None else plan.set_rays(rays)


def run_full(plan, seeds, rays, exact=False, **grid):
    """[block 0, block 1, ...] and the fetch of one run of the plan in spectra mode with ASE seeds."""
    set_rays(plan, rays, **grid).set_exact_emission(exact).enable_spectra().set_spectra_ase_seeds(seeds).run()
    info = plan.fetch()
    full = plan.fetch_full_spectra()
    return [full["ase"]] + full["seeds"], info


def plain_spectra(hip, q, rays, exact=False, key=None, **grid):
    """The rows of a plain spectra plan of problem q (an emission problem, or one created with a seed); with a key once per key."""
    if key is not None and key in _plain:
        return _plain[key][1]
    with hip.Plan(q) as plan:
        out = set_rays(plan, rays, **grid).set_exact_emission(exact).enable_spectra().run().fetch_spectra()
    if key is not None:
        _plain[key] = (q, out)
    return out


def gate_block(blk, ref, tier, label):
    """One block of rows against the oracle: check_against, the tier, no clean row left out.  Returns the per-ray rel-L2."""
    rows, nzero = check_against(blk, ref, label)
    assert rows + nzero == int((ref["err"] == 0).sum()), label      # no row with err = 0 in the oracle is left out
    ok = ref["err"] == 0
    l2 = row_figures(blk["Iv"][ok], ref["Iv"][ok])[0]
    note(f"{label}: worst per-ray rel-L2 {l2:.3e} (tier {tier:g})")
    assert l2 < tier, (label, l2)
    return l2


def gate_blocks(blocks, refs, exact, label):
    assert len(blocks) == len(refs)
    gate_block(blocks[0], refs[0], TIGHT_TIER if exact else DEFAULT_TIER, f"{label} / block 0 (ASE)")
    for s in range(1, len(blocks)):
        gate_block(blocks[s], refs[s], TIGHT_TIER, f"{label} / block {s} (seed {s - 1})")


def bits_differ(a, b, label):
    """Elements of two spectra that are not the same double (expected: 0), noted before the caller asserts."""
    diff = a["Iv"].view(np.uint64) != b["Iv"].view(np.uint64)
    both = (b["Iv"] != 0) & np.isfinite(b["Iv"]) & np.isfinite(a["Iv"])
    rel = float((np.abs(a["Iv"] - b["Iv"])[both] / np.abs(b["Iv"])[both]).max()) if both.any() else 0.0
    note(f"{label}: differing elements {int(diff.sum())} of {diff.size} in {int(diff.any(axis=1).sum())} rows, max rel diff {rel:.3e}")
    return int(diff.sum())


def same_rows(a, b, label):
    assert np.array_equal(a["err"], b["err"]), label
    assert a["ray2"].tobytes() == b["ray2"].tobytes(), label
    assert bits_differ(a, b, label) == 0, label


def check_report(info, err_blocks, rays, label):
    """failure_code is the OR of the codes over every block; every ray failing in any block is reported once (more than
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


# ---------------------------------------------------------------------------------------------- 1. every block against the oracle
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_every_block_against_the_oracle(hip, oracle, ase_small, method, N, mode, exact):
    """N = 3 takes rt_spec_ase_seeds_kernel<6>, N = 5 the generic instance."""
    p = S.problem_of(ase_small, method, N)
    seeds = S.seeds_of(p)
    rays = p.build_rays()
    refs = S.refs(oracle, p, seeds, rays, ("main", method, N))
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, seeds, None if mode == "grid" else rays, exact)
        assert info["stats"]["n_rays"] == len(rays) and plan.last_fused() is False and info["image"] is None
        assert not plan.last_march_instance() & (8 << 1)                      # the march of spectra mode, not the scan instance
    assert len(blocks) == 3 and info["failure_code"] == 0 and len(info["failed_rays"]) == 0
    gate_blocks(blocks, refs, exact, f"spectra with ASE seeds / method {method}, N = {N}, ray {mode}, {'exact' if exact else 'default'} emission")
    assert blocks[0]["ray2"].tobytes() == blocks[1]["ray2"].tobytes() == blocks[2]["ray2"].tobytes()
    assert all(b["Iv"].any() for b in blocks)
    assert not np.array_equal(blocks[1]["Iv"].any(axis=1), blocks[2]["Iv"].any(axis=1))         # the seeds light different rays
    assert not np.array_equal(blocks[0]["Iv"], blocks[1]["Iv"])


# ---------------------------------------------------------------------------------------------- 2. bit-equal to the plans it replaces
@pytest.mark.parametrize("mode", ["grid", "list"])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_blocks_equal_the_plain_plan_and_the_plans_created_with_the_seeds(hip, ase_small, method, N, mode):
    p = S.problem_of(ase_small, method, N)
    seeds = S.seeds_of(p)
    rays = None if mode == "grid" else p.build_rays()
    label = f"spectra with ASE seeds / method {method}, N = {N}, ray {mode}"
    with hip.Plan(p) as plan:
        plain = {exact: set_rays(plan, rays).set_exact_emission(exact).enable_spectra().run().fetch_spectra() for exact in (False, True)}
        runs = {exact: run_full(plan, seeds, rays, exact)[0] for exact in (False, True)}
    assert plain[False]["Iv"].tobytes() != plain[True]["Iv"].tobytes()                          # (the two emission modes are two arithmetics)
    for exact in (False, True):
        same_rows(runs[exact][0], plain[exact], f"{label}, {'exact' if exact else 'default'} emission / block 0 against the same plan without seeds")
    for s, sd in enumerate(seeds):
        one = plain_spectra(hip, A.carry(p, sd), rays, key=("carry", method, N, mode, s))
        for exact in (False, True):                                                             # (the seed blocks know nothing of the emission mode)
            same_rows(runs[exact][1 + s], one, f"{label} / block {1 + s} against the spectra plan created with seed {s}")


# ---------------------------------------------------------------------------------------------- 3. mixed tiles
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_block_0_on_mixed_tiles(hip, oracle, ase_small, method, N):
    """update_regimes' composed list of the cap_split regime: tiles of the small, the regular and the irregular branch and mixed
    ones.  What catches a contraction of the emission update that moved, or a tile-wide choice taken over other lanes."""
    c = ur.case(oracle, ase_small, "cap_split", N, method)
    p, rays = c.p, c.rays
    seeds = A.seeds_of(p)
    names = [name for name, _, _ in c.tiles]
    assert len(names) >= 4 and len(rays) % 64 == ur.RAGGED
    label = f"spectra with ASE seeds, mixed tiles / {c.label}"
    with hip.Plan(p) as plan:
        plain = {exact: plan.set_rays(rays).set_exact_emission(exact).enable_spectra().run().fetch_spectra() for exact in (False, True)}
        runs = {exact: run_full(plan, seeds, rays, exact)[0] for exact in (False, True)}
    for exact in (False, True):
        same_rows(runs[exact][0], plain[exact], f"{label}, {'exact' if exact else 'default'} emission / block 0 against the same plan without seeds")
    for s, sd in enumerate(seeds):
        same_rows(runs[False][1 + s], plain_spectra(hip, A.carry(p, sd), rays), f"{label} / block {1 + s} against the spectra plan created with seed {s}")
        assert runs[False][1 + s]["Iv"].tobytes() == runs[True][1 + s]["Iv"].tobytes()


# ---------------------------------------------------------------------------------------------- 4. F_SKIP
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_rays_with_all_sums_zero_are_dark_in_block_0_and_lit_under_the_seeds(hip, oracle, ase_small, method, N):
    """The dark variant: the emission march marks a ray whose every sum is zero (F_SKIP).  It has a row of zeros in block 0 and
    carries f0_s f_s[4][k] exp(0) under every seed; whole tiles lie in the dark: they skip the recurrence and run the seed half."""
    p = S.problem_of(ase_small, method, N, dark=True)
    seeds = S.seeds_of(p)
    rays = p.build_rays()
    refs = S.refs(oracle, p, seeds, rays, ("dark", method, N))
    zero = S.all_zero_sums(refs[0])
    tiles = S.dark_tiles(zero)
    label = f"spectra with ASE seeds, dark / method {method}, N = {N}"
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, seeds, None)
        print(f"{label}: n_skipped {info['stats']['n_skipped']}, rays with all sums zero on the oracle {int(zero.sum())}")
        assert info["stats"]["n_skipped"] >= 300 and int(zero.sum()) >= 300 and info["failure_code"] == 0
        plain = plan.set_spectra_ase_seeds([]).run().fetch_spectra()
    gate_blocks(blocks, refs, False, label)
    same_rows(blocks[0], plain, f"{label} / block 0 against the same plan without seeds")
    assert not blocks[0]["Iv"][zero].any() and blocks[0]["Iv"][~zero].any(axis=1).all()
    lit = zero & refs[1]["Iv"].any(axis=1)
    assert int(lit.sum()) >= 150 and blocks[1]["Iv"][lit].any(axis=1).all()                      # zeros in block 0, non-zero under `wide`
    assert len(tiles) >= 2 and any(lit[t:t + 64].any() for t in tiles)                          # the wholly dark tiles among them
    for s, sd in enumerate(seeds):
        one = plain_spectra(hip, A.carry(p, sd), None)
        same_rows(blocks[1 + s], one, f"{label} / block {1 + s} against the spectra plan created with seed {s}")
        for t in tiles:
            assert blocks[1 + s]["Iv"][t:t + 64].tobytes() == one["Iv"][t:t + 64].tobytes()


# ---------------------------------------------------------------------------------------------- 5. codes
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_a_negative_seed_fails_in_its_own_block_only(hip, oracle, ase_small, method, N):
    """negative(narrow): -2 in block 2 alone, on more rays than the report holds: every one once, the first in list order."""
    p = S.problem_of(ase_small, method, N)
    seeds = S.negative_pair(p)
    rays = p.build_rays()
    refs = S.refs(oracle, p, seeds, rays, ("negative", method, N))
    assert [S.code_of(r["err"]) for r in refs] == [0, 0, 1 << 2] and int((refs[2]["err"] != 0).sum()) > cabi.RT_N_FAILED_MAX
    for mode_rays in (None, rays):
        with hip.Plan(p) as plan:
            blocks, info = run_full(plan, seeds, mode_rays)
        label = f"spectra with ASE seeds, negative(narrow) / method {method}, N = {N}, ray {'grid' if mode_rays is None else 'list'}"
        gate_blocks(blocks, refs, False, label)
        assert [S.code_of(b["err"]) for b in blocks] == [0, 0, 1 << 2]
        check_report(info, [r["err"] for r in refs], rays, label)


@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_a_nan_in_a_lineshape_table_fails_per_block_where_the_oracle_has_it(hip, oracle, ase_small, method, N):
    p = S.nan_tables(S.problem_of(ase_small, method, N))
    seeds = S.seeds_of(p)
    rays = p.build_rays()
    refs = S.refs(oracle, p, seeds, rays, ("nan", method, N))
    assert [S.code_of(r["err"]) for r in refs] == [1 << 3] * 3
    for exact in (False, True):
        with hip.Plan(p) as plan:
            blocks, info = run_full(plan, seeds, rays, exact)
        label = f"spectra with ASE seeds, a NaN lineshape value / method {method}, N = {N}, {'exact' if exact else 'default'} emission"
        gate_blocks(blocks, refs, exact, label)
        for b, r in zip(blocks, refs):
            assert np.array_equal(b["err"], r["err"]) and int((b["err"] == -3).sum()) >= 20
        check_report(info, [r["err"] for r in refs], rays, label)


@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_a_steep_ray_fails_in_every_block(hip, oracle, ase_small, method, N):
    """One ray launched almost perpendicular to z (s.z^2 < 0.01, Helper.h:515): error -1 and zeros in every block, reported once."""
    p = S.problem_of(ase_small, method, N)
    seeds = S.seeds_of(p)
    bad = S.steep(p.build_rays())
    refs = [oracle.probe(p, bad, want_Iv=True)] + [oracle.probe(A.carry(p, sd), bad, want_Iv=True) for sd in seeds]
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, seeds, bad)
    for r, (blk, ref) in enumerate(zip(blocks, refs)):
        assert ref["err"][7] == -1 and blk["err"][7] == -1 and not blk["Iv"][7].any()
        assert all(blk["ray2"][k][7] == 0 for k in "xyab")
        check_against(blk, ref, f"spectra with ASE seeds, a steep ray / method {method}, N = {N} / block {r}")
    assert info["failure_code"] == 1 << 1 and len(info["failed_rays"]) == 1 and info["failed_rays"][0] == bad[7]


# ---------------------------------------------------------------------------------------------- 6. shapes where the stores can go wrong
@pytest.mark.parametrize("n_rays", [1, 64])
@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_one_ray_and_one_full_tile(hip, oracle, ase_small, method, N, n_rays):
    p = S.problem_of(ase_small, method, N)
    seeds = S.seeds_of(p)
    rays = p.build_rays()[611:611 + n_rays].copy()
    refs = S.refs(oracle, p, seeds, rays, ("rays", method, N, n_rays))
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, seeds, rays)
    assert info["stats"]["n_rays"] == n_rays and all(b["Iv"].shape == (n_rays, p.beam.nv) for b in blocks)
    gate_blocks(blocks, refs, False, f"spectra with ASE seeds / method {method}, N = {N}, {n_rays} ray(s)")


@pytest.mark.parametrize("method", METHODS)
def test_an_odd_number_of_frequencies(hip, oracle, ase_small, method):
    """An odd K (the construction of tests/test_gpu_length_spectra.py): no 16-byte store is aligned, every row leaves by the 8-byte path."""
    p = S.odd_k(ase_small, method)
    assert p.beam.nv == 51 and p.use_emis
    seeds = S.seeds_of(p)
    rays = p.build_rays()
    refs = S.refs(oracle, p, seeds, rays, ("K51", method))
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, seeds, None, first=0, stride=1)
        plain = plan.set_spectra_ase_seeds([]).run().fetch_spectra()
    assert info["failure_code"] == 0 and all(b["Iv"].shape == (len(rays), 51) for b in blocks)
    gate_blocks(blocks, refs, False, f"spectra with ASE seeds / method {method}, K = 51")
    same_rows(blocks[0], plain, f"spectra with ASE seeds / method {method}, K = 51 / block 0 against the same plan without seeds")


@pytest.mark.parametrize("N", [3, 5])
@pytest.mark.parametrize("method", METHODS)
def test_one_seed(hip, oracle, ase_small, method, N):
    """n_seed = 1: two blocks, the second the rows of the plan created with that seed."""
    p = S.problem_of(ase_small, method, N)
    narrow = S.seeds_of(p)[1]
    rays = p.build_rays()
    refs = S.refs(oracle, p, S.seeds_of(p), rays, ("main", method, N))
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, (narrow,), rays)
    assert len(blocks) == 2 and info["failure_code"] == 0
    gate_blocks(blocks, [refs[0], refs[2]], False, f"spectra with ASE seeds / method {method}, N = {N}, n_seed = 1")
    same_rows(blocks[1], plain_spectra(hip, A.carry(p, narrow), rays), f"spectra with ASE seeds / method {method}, N = {N}, n_seed = 1 against the plan created with it")


@pytest.mark.parametrize("method", METHODS)
def test_a_strided_device_grid(hip, oracle, ase_small, method):
    p = S.problem_of(ase_small, method, 3)
    seeds = S.seeds_of(p)
    rays = p.build_rays(np.arange(3, p.n_rays_total, 7, dtype=np.int64))
    assert len(rays) % 64 != 0
    refs = S.refs(oracle, p, seeds, rays, ("strided", method))
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, seeds, None, first=3, stride=7)
    assert info["stats"]["n_rays"] == len(rays)
    gate_blocks(blocks, refs, False, f"spectra with ASE seeds / method {method}, grid first 3 stride 7")


@pytest.mark.parametrize("method", METHODS)
def test_a_list_behind_a_grid_and_a_grid_behind_a_list_on_one_plan(hip, oracle, ase_small, method):
    """On a forward ray grid the seed factors come from per-seed tables of the grid's points, on a list from the seed factor at the
    launch ray: the ray set of the RUN decides.  The list is the grid's rays reversed -- a run that still indexed the grid's
    tables would give ray t the factor of grid point t."""
    p = S.problem_of(ase_small, method, 3)
    seeds = S.seeds_of(p)
    rays = p.build_rays()
    back = np.ascontiguousarray(rays[::-1])
    refs = S.refs(oracle, p, seeds, rays, ("main", method, 3))
    rrefs = S.refs(oracle, p, seeds, back, ("reversed", method))
    with hip.Plan(p) as plan:
        on_grid, _ = run_full(plan, seeds, None)
        plan.set_rays(back).run()
        full = plan.fetch_full_spectra()
        on_list = [full["ase"]] + full["seeds"]
        plan.set_ray_grid().run()
        full = plan.fetch_full_spectra()
        again = [full["ase"]] + full["seeds"]
    gate_blocks(on_list, rrefs, False, f"spectra with ASE seeds / method {method}, a list behind a grid")
    gate_blocks(again, refs, False, f"spectra with ASE seeds / method {method}, a grid behind a list")
    for a, b in zip(again, on_grid):
        assert a["Iv"].tobytes() == b["Iv"].tobytes() and a["err"].tobytes() == b["err"].tobytes()


# ---------------------------------------------------------------------------------------------- 7. state
@pytest.mark.parametrize("method", METHODS)
def test_block_0_is_served_by_the_plain_accessors_and_the_tensors_view_the_rows(hip, ase_small, method):
    p = S.problem_of(ase_small, method, 3)
    seeds = S.seeds_of(p)
    nr, K = p.n_rays_total, p.beam.nv
    with hip.Plan(p) as plan:
        blocks, _ = run_full(plan, seeds, None)
        plain = plan.fetch_spectra()
        for key in ("Iv", "ray2", "err"):
            assert plain[key].tobytes() == blocks[0][key].tobytes(), key
        ptrs = [plan.full_spectra_ptrs(r) for r in range(3)]
        assert plan.spectra_ptr() == ptrs[0][0]
        for r in (1, 2):
            assert ptrs[r][0] == ptrs[0][0] + 8 * r * nr * K                                    # block-major
            assert ptrs[r][1] == ptrs[0][1]                                                     # one ray2
            assert ptrs[r][2] == ptrs[0][2] + 4 * r * nr
        views = plan.full_spectra_tensors()
        assert tuple(views["Iv"].shape) == (3, nr, K) and tuple(views["err"].shape) == (3, nr) and tuple(views["ray2"].shape) == (nr, 4)
        assert views["Iv"].data_ptr() == plan.spectra_ptr()
        iv, er, r2 = views["Iv"].cpu().numpy(), views["err"].cpu().numpy(), views["ray2"].cpu().numpy()
        for r in range(3):
            assert np.array_equal(iv[r], blocks[r]["Iv"], equal_nan=True) and np.array_equal(er[r], blocks[r]["err"])
        assert np.array_equal(r2.view(np.uint32), cabi.rays_to_array(blocks[0]["ray2"]).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("method", METHODS)
def test_removing_the_seeds_restores_the_plain_plan(hip, ase_small, method):
    """set_spectra_ase_seeds([]) and enable_spectra(False) leave plain spectra mode bit for bit (no atomics on data); a rejected
    call leaves the installed seeds."""
    p = S.problem_of(ase_small, method, 3)
    seeds = S.seeds_of(p)
    lib = hip.HipLibrary.get().lib
    with hip.Plan(p) as fresh:
        want = fresh.set_ray_grid().enable_spectra().run().fetch_spectra()
    with hip.Plan(p) as plan:
        with_seeds, _ = run_full(plan, seeds, None)
        arr = (cabi.RtSeed * 3)()
        assert lib.rt_hip_plan_set_spectra_ase_seeds(plan._h, 3, arr) == cabi.RT_ERR_ARG and b"more than RT_N_SEED_MAX" in lib.rt_hip_last_error()
        assert lib.rt_hip_plan_set_spectra_ase_seeds(plan._h, 1, arr) == cabi.RT_ERR_ARG and b"incomplete seed table" in lib.rt_hip_last_error()
        full = plan.run().fetch_full_spectra()
        for a, b in zip([full["ase"]] + full["seeds"], with_seeds):
            assert a["Iv"].tobytes() == b["Iv"].tobytes() and a["err"].tobytes() == b["err"].tobytes()
        got = plan.set_spectra_ase_seeds([]).run().fetch_spectra()
        for key in ("Iv", "ray2", "err"):
            assert want[key].tobytes() == got[key].tobytes(), key
        with pytest.raises(hip.RayTraceError, match="ASE seeds"):
            plan.full_spectra_ptrs(0)
        plan.set_spectra_ase_seeds(seeds).enable_spectra(False)                                  # drops the seeds
        assert plan._n_spec_ase_seed == 0
        got = plan.enable_spectra().run().fetch_spectra()
        for key in ("Iv", "ray2", "err"):
            assert want[key].tobytes() == got[key].tobytes(), key
        with pytest.raises(hip.RayTraceError, match="ASE seeds"):
            plan.full_spectra_ptrs(0)
        img = plan.enable_spectra(False).run().fetch()                                           # ... and image mode runs again
        assert img["failure_code"] == 0 and img["image"] is not None


@pytest.mark.parametrize("method", METHODS)
def test_update_gain_keeps_the_seeds(hip, oracle, ase_small, method):
    p = S.problem_of(ase_small, method, 3)
    seeds = S.seeds_of(p)
    key = ("tables_b", method)
    if key not in S._built:
        S._built[key] = (p, tv.tables_b(p))
    pb = S._built[key][1]
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        before, _ = run_full(plan, seeds, None)
        plan.update_gain(pb.gain).run()
        info = plan.fetch()
        full = plan.fetch_full_spectra()
    after = [full["ase"]] + full["seeds"]
    assert len(after) == 3 and info["failure_code"] == 0
    assert not np.array_equal(before[0]["Iv"], after[0]["Iv"]) and not np.array_equal(before[1]["Iv"], after[1]["Iv"])
    gate_blocks(after, S.refs(oracle, pb, seeds, rays, ("tables_b", method)), False, f"spectra with ASE seeds after update_gain (tables B) / method {method}")


def test_refusals(hip, ase_small):
    lib = hip.HipLibrary.get().lib
    ARG = cabi.RT_ERR_ARG

    def refused(rc, *words):
        text = lib.rt_hip_last_error()
        assert rc == ARG and all(w in text for w in words), (rc, text)

    p = S.problem_of(ase_small, 2, 5)
    seeds, arr, _keep = hip._seed_array(S.seeds_of(p), "test", "test")
    set_ = lib.rt_hip_plan_set_spectra_ase_seeds
    refused(set_(None, 1, arr), b"rt_hip_plan_set_spectra_ase_seeds", b"NULL plan")
    with hip.Plan(A.carry(p, seeds[0])) as plan:                                               # a plan created with a seed
        plan.set_ray_grid().enable_spectra()
        refused(set_(plan._h, 1, arr), b"created with a seed", b"rt_hip_plan_set_spectra_seeds")
    q = copy.copy(p)
    q.gain = [rt.Gain(g.x, g.y, g.n, g.g0, None, g.gv, g.Nv) for g in p.gain]
    q = mp.with_method(q, 2)
    assert not q.use_emis and q.seed is None
    with hip.Plan(q) as plan:                                                                   # neither a seed nor E0
        plan.set_ray_grid().enable_spectra()
        refused(set_(plan._h, 1, arr), b"not an emission plan", b"tables without E0")
    with hip.Plan(p) as plan:
        plan.set_ray_grid()
        refused(set_(plan._h, 2, arr), b"spectra mode is off", b"rt_hip_plan_enable_spectra first")
        plan.enable_step()
        refused(set_(plan._h, 2, arr), b"spectra mode is off")
        plan.enable_step(False).enable_length_spectra()
        refused(set_(plan._h, 2, arr), b"length spectra are on", b"per-ray ASE seeds at every length are not built")
        plan.enable_length_spectra(False).enable_spectra()
        refused(set_(plan._h, 3, arr), b"more than RT_N_SEED_MAX")
        refused(set_(plan._h, -1, arr), b"n_seed must be 0 .. RT_N_SEED_MAX")
        refused(set_(plan._h, 2, None), b"NULL seeds")
        refused(set_(plan._h, 1, (cabi.RtSeed * 1)()), b"incomplete seed table")
        assert set_(plan._h, 0, None) == 0                                                      # (removing what is not there)
        refused(lib.rt_hip_plan_fetch_full_spectra(plan._h, 0, None, None, None), b"not a spectra run with ASE seeds")     # has not run
        plan.run()
        refused(lib.rt_hip_plan_fetch_full_spectra(plan._h, 0, None, None, None), b"not a spectra run with ASE seeds")     # ran without seeds
        # the old refusal of the seeded installer stands, word for word
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 1, arr), b"created without a seed", b"ASE seeds are not built")
        plan.set_spectra_ase_seeds(seeds).run()
        for r in (-1, 3):
            refused(lib.rt_hip_plan_fetch_full_spectra(plan._h, r, None, None, None), b"r must be 0 .. n_seed")
            refused(lib.rt_hip_plan_full_spectra_ptrs(plan._h, r, None, None, None), b"r must be 0 .. n_seed")
        assert lib.rt_hip_plan_fetch_full_spectra(plan._h, 2, None, None, None) == 0            # any pointer may be NULL
        assert lib.rt_hip_plan_full_spectra_ptrs(plan._h, 2, None, None, None) == 0
        refused(lib.rt_hip_plan_fetch_seed_spectra(plan._h, 0, None, None, None), b"not a spectra run with spectra seeds")
        refused(lib.rt_hip_plan_set_spectra_seeds(plan._h, 1, arr), b"created without a seed", b"ASE seeds are not built")
        # while the seeds are installed spectra mode is on: every switch and installer refuses as it always has
        for call, word in ((plan.enable_step, "spectra mode"), (plan.enable_path, "spectra mode"), (plan.enable_length_spectra, "spectra mode"),
                           (plan.enable_length_scan, "spectra mode"), (lambda: plan.set_ase_seeds(seeds), "spectra mode")):
            with pytest.raises(hip.RayTraceError, match=word):
                call()
        assert lib.rt_hip_plan_set_ase_seeds(plan._h, 0, None, None) == 0                       # (no ASE seeds of step mode to remove: these stay)
        full = plan.run().fetch_full_spectra()
        assert len(full["seeds"]) == 2 and full["seeds"][0]["Iv"].any()


# ---------------------------------------------------------------------------------------------- 8. the one-call form
@pytest.mark.parametrize("method", METHODS)
def test_the_one_call_form_equals_the_plans_rows(hip, ase_small, method):
    p = S.problem_of(ase_small, method, 3)
    seeds = S.seeds_of(p)
    rays = p.build_rays()
    with hip.Plan(p) as plan:
        blocks, info = run_full(plan, seeds, rays)
    out = hip.calc_rays_ase_seeds(p, seeds, rays)
    assert out["failure_code"] == info["failure_code"] == 0 and len(out["seeds"]) == 2 and len(out["failed_rays"]) == 0
    assert out["stats"]["cell_steps"] == info["stats"]["cell_steps"] and out["stats"]["n_rays"] == len(rays)
    for a, b in zip([out["ase"]] + out["seeds"], blocks):
        for key in ("Iv", "ray2", "err"):
            assert a[key].tobytes() == b[key].tobytes(), key
    # an [n][4] float64 array is taken as calc_rays takes it
    again = hip.calc_rays_ase_seeds(p, seeds[1:], cabi.rays_to_array(rays[:70]).astype(np.float64))
    assert len(again["seeds"]) == 1 and again["ase"]["Iv"].shape == again["seeds"][0]["Iv"].shape == (70, p.beam.nv)
    assert again["ase"]["Iv"].tobytes() == blocks[0]["Iv"][:70].tobytes()
