"""The two (method, seed) pairs that Problem.method never produces, through every mode of the HIP path.

    forward ASE       no seed, method 2: emission (`EMIS`), deposit at the exit ray (negated angles, y mirrored where
                      beam.y[0] >= 0); march instance mode 0 (P.method and P.use_emis read at run time); evl in slots 1..S
    backward seeded   a seed, method 1: gain-only, seed_factor at the EXIT ray per ray (no seed table), deposit at the launch
                      ray; on the beam's own grid the pixel comes from the grid index (FQ_OWN_CELLS) in the gain-only kernel

The comparison target is the oracle, which tests/test_oracle_pin.py pins bit for bit to the reference on both pairs
(tests/golden/ASE_small_fwd_ref.npz, seed_small_bwd_ref.npz); those fixtures are compared here directly as well.

Gates (tests/element_gate.py; nothing new): image and I_ang element by element at DEFAULT_TIER (1e-5) for default
emission, TIGHT_TIER (1e-11) for gain-only and set_exact_emission(True), "reordering" between two device runs; the march
record bit for bit (same_record of tests/test_gpu_edges.py); path positions bit for bit, intensities at rtol 2e-6; spectra
per ray as tests/test_gpu_spectra.py gates them (check_against).  Counts always from counts_from_oracle with explicit rays.
Every figure is printed before its assertion, and so are the counts behind the conditions (ELEMENT_PARITY_FILE appends
them to a file: profiles/method_pairs_parity.txt)."""
import copy
import importlib

import numpy as np
import pytest

import method_pairs as mp
from conftest import GOLDEN
from element_gate import DEFAULT_TIER, TIGHT_TIER, counts_from_oracle, gate_outputs, note
from test_gpu_edges import same_outputs_in_a_failing_run, same_record
from test_gpu_spectra import check_against
from test_gpu_step import _ray_set, gate_step, image_then_step, reduced

rt = importlib.import_module("raytrace-miniapp_amd")
problem_mod = importlib.import_module("raytrace-miniapp_amd.problem")
pytestmark = pytest.mark.gpu

PAIRS = ["fwd_ase", "bwd_seed"]
FIXTURE = {"fwd_ase": "ASE_small_fwd_ref.npz", "bwd_seed": "seed_small_bwd_ref.npz"}


# ---------------------------------------------------------------------------------------------- helpers
_base = {}


def pair_problem(pair, ase_small, seed_small):
    """The shipped input of the pair with the other method, one object per session."""
    if pair not in _base:
        _base[pair] = mp.ase_forward(ase_small) if pair == "fwd_ase" else mp.seed_backward(seed_small)
    p = _base[pair]
    assert p.method == (2 if pair == "fwd_ase" else 1) and (p.seed is None) == (pair == "fwd_ase")
    return p


def tier_of(p, exact=False):
    return TIGHT_TIER if (exact or not p.use_emis) else DEFAULT_TIER


def list_ids(pair, n):
    """(a): ids 200000 + arange(n) of ASE_small's grid, every 7 803rd ray of seed_small's."""
    return (200000 + np.arange(n, dtype=np.int64)) if pair == "fwd_ase" else np.arange(n, dtype=np.int64) * 7803


def run_plan(hip, p, rays=None, probe=False, exact=False, grid=None):
    """One plan run: rays a list, or None for the problem's ray grid (grid = dict(first, stride) for part of it)."""
    with hip.Plan(p) as plan:
        if rays is None:
            plan.set_ray_grid(**(grid or {}))
        else:
            plan.set_rays(rays)
        if probe:
            plan.enable_probe()
        if exact:
            plan.set_exact_emission(True)
        out = plan.run().fetch()
        out["fused"] = plan.last_fused()
        if probe:
            out["probe"] = plan.fetch_probe()
    return out


def oracle_of(oracle, p, rays, n_threads=4):
    """(image_loop, counts) of the oracle on explicit rays."""
    return oracle.image_loop(p, rays, n_threads=n_threads), counts_from_oracle(oracle, p, rays, n_threads=n_threads)


def against_the_oracle(hip, oracle, p, rays, label, exact=False, probe=True):
    """A list through a plan with the probe: record bit for bit, cell_steps and failure_code equal, image and I_ang gated."""
    out = run_plan(hip, p, rays, probe=probe, exact=exact)
    ref, counts = oracle_of(oracle, p, rays)
    if probe:
        ora = oracle.probe(p, rays, want_Iv=False)
        same_record(out["probe"], ora)
        ok = ora["err"] == 0
        for key in "xyab":
            assert np.array_equal(out["probe"]["ray2"][key][ok].view(np.uint32), ora["ray2"][key][ok].view(np.uint32)), (label, key)
    assert out["stats"]["n_rays"] == len(rays), label
    assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"], label
    assert out["failure_code"] == ref["failure_code"], label
    note(f"{label}: {len(rays)} rays, {int(counts[0].sum())} deposit in the image, {int(counts[1].sum())} in I_ang, "
         f"non-zero image elements of the oracle {int(np.count_nonzero(ref['image']))} of {ref['image'].size}, one launch {out['fused']}")
    gate_outputs(out, ref, p, counts, tier_of(p, exact), label)
    return out, ref, counts


def with_lengths(p, N):
    """N lengths, tables repeated as test_other_numbers_of_lengths (tests/test_gpu_edges.py) repeats them."""
    q = copy.copy(p)
    g = p.gain
    q.gain = [g[0]] + [g[1 + (i % 2)] for i in range(N - 1)]
    return q


def grid_problem(pair, ase_small, seed_small):
    """(b): the device-generated grids, 1 440 and 1 350 rays."""
    p = pair_problem(pair, ase_small, seed_small)
    if pair == "fwd_ase":
        return problem_mod.regrid_beam(p, nx=12, ny=6, na=5, nb=4)
    return problem_mod.regrid_seed_beam(p, nx=9, ny=5, na=6, nb=5)


# ---------------------------------------------------------------------------------------------- a. ray lists, ragged
@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("pair", PAIRS)
def test_ragged_ray_lists(hip, oracle, ase_small, seed_small, pair, n):
    p = pair_problem(pair, ase_small, seed_small)
    rays = p.build_rays(list_ids(pair, n))
    out, ref, _ = against_the_oracle(hip, oracle, p, rays, f"pairs a: {pair}, {n} rays")
    assert not out["fused"]
    if n == 1000:
        assert np.count_nonzero(ref["image"]) > 5000            # (8 996 and 58 630 on the CPU)


@pytest.mark.parametrize("pair", PAIRS)
def test_every_97th_ray_against_the_reference_fixture(hip, oracle, ase_small, seed_small, pair):
    p = pair_problem(pair, ase_small, seed_small)
    fx = np.load(GOLDEN / FIXTURE[pair])
    rays = p.build_rays(mp.strided_ids(p, int(fx["stride"])))
    assert len(rays) == int(fx["n_rays"]) == (4114 if pair == "fwd_ase" else 80444) and int(fx["method"]) == p.method
    out, ref, counts = against_the_oracle(hip, oracle, p, rays, f"pairs a: {pair}, every 97th ray against the oracle", probe=False)
    assert out["failure_code"] == int(fx["failure_code"]) == 0
    assert np.count_nonzero(fx["image"]) > fx["image"].size // 2     # (oracle == fixture bit for bit: tests/test_oracle_pin.py)
    gate_outputs(out, dict(image=fx["image"], I_ang=fx["I_ang"]), p, counts, tier_of(p), f"pairs a: {pair}, every 97th ray against the reference's CPU loop")


# ---------------------------------------------------------------------------------------------- b. device-generated grids
@pytest.mark.parametrize("pair", PAIRS)
def test_device_generated_grids(hip, oracle, ase_small, seed_small, pair):
    p = grid_problem(pair, ase_small, seed_small)
    rays = p.build_rays()
    ref, counts = oracle_of(oracle, p, rays)
    dep_img, dep_ang, nz = int(counts[0].sum()), int(counts[1].sum()), int(np.count_nonzero(ref["image"]))
    note(f"pairs b: {pair} grid, {len(rays)} rays, {dep_img} deposit in the image, {dep_ang} in I_ang, {nz} non-zero image elements")
    if pair == "fwd_ase":     # the out-of-range branch of the angle cell is taken by two rays of three
        assert (len(rays), dep_img, dep_ang) == (1440, 1429, 463)
    else:
        assert (len(rays), dep_img, dep_ang, nz) == (1350, 1350, 1350, 3444)
    grid = run_plan(hip, p)
    lst = run_plan(hip, p, rays)
    assert not grid["fused"] and not lst["fused"]
    note(f"pairs b: {pair} grid, one launch taken: {grid['fused']}")
    for out, what in ((grid, "grid"), (lst, "list")):
        assert out["failure_code"] == ref["failure_code"] == 0 and out["stats"]["n_rays"] == len(rays)
        assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"]
        gate_outputs(out, ref, p, counts, tier_of(p), f"pairs b: {pair}, ray {what} against the oracle")
    gate_outputs(grid, lst, p, counts, "reordering", f"pairs b: {pair}, ray grid against the same rays as a list")
    # part of the grid: first 3, stride 7 (a ragged last tile)
    ids = np.arange(3, p.n_rays_total, 7, dtype=np.int64)
    part_ref, part_counts = oracle_of(oracle, p, p.build_rays(ids))
    part = run_plan(hip, p, grid=dict(first=3, stride=7))
    assert part["stats"]["n_rays"] == len(ids) and part["stats"]["cell_steps"] == part_ref["counters"]["cell_steps"]
    gate_outputs(part, part_ref, p, part_counts, tier_of(p), f"pairs b: {pair}, ray grid first 3 stride 7 against the oracle")


def test_forward_ase_keeps_two_kernels_where_backward_takes_one(hip, oracle, ase_small):
    """32 rays per pixel on the beam's own grid: method 1 takes the one launch (the control), method 2 must not -- its
    deposit is at the exit ray, the few-runs deposit of the one launch is by the launch pixel."""
    back = problem_mod.regrid_beam(ase_small, nx=6, ny=4, na=8, nb=4)
    p = mp.with_method(back, 2)
    control = run_plan(hip, back)
    assert control["fused"], "the control did not take the one launch: this grid no longer shows what it is meant to show"
    rays = p.build_rays()
    ref, counts = oracle_of(oracle, p, rays)
    out = run_plan(hip, p)
    note(f"pairs b: forward ASE on a 32-rays-per-pixel grid, one launch taken: {out['fused']} (backward: {control['fused']}); "
         f"{int(counts[0].sum())} of {len(rays)} rays deposit in the image, {int(counts[1].sum())} in I_ang")
    assert not out["fused"]
    assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"] and out["failure_code"] == 0
    assert int(counts[0].sum()) < len(rays) and int(counts[1].sum()) < len(rays) // 2
    gate_outputs(out, ref, p, counts, DEFAULT_TIER, "pairs b: forward ASE, 6 x 4 x 8 x 4 grid against the oracle")
    assert not np.array_equal(out["image"], control["image"])


# ---------------------------------------------------------------------------------------------- c. backward seeded, own grid
_wide = {}


def wide_problems(seed_small):
    if not _wide:
        _wide["full"] = mp.seed_backward(mp.wide_seed(seed_small))
        _wide["small"] = mp.seed_backward(mp.wide_seed(problem_mod.regrid_beam(seed_small, nx=7, ny=5, na=6, nb=5)))
    return _wide["full"], _wide["small"]


def test_backward_seeded_on_the_beams_own_grid(hip, oracle, seed_small, monkeypatch):
    """The own-cell deposit (pixel and angle cell from the grid index) inside the gain-only kernel."""
    full, small = wide_problems(seed_small)
    assert full.method == 1 and full.n_rays_total == 399000
    for g, h in zip(full.ray_grid, (full.beam.x, full.beam.y, full.beam.a, full.beam.b)):
        assert np.array_equal(g, h)
    rays = full.build_rays(mp.strided_ids(full, 7))
    out, ref, counts = against_the_oracle(hip, oracle, full, rays, "pairs c: backward seeded, wide seed, every 7th ray of the beam's grid", probe=False)
    assert np.count_nonzero(ref["image"]) == 102254 and ref["image"].size == 123000
    # the whole small grid, generated on the device
    assert small.n_rays_total == 1050
    rays = small.build_rays()
    ref, counts = oracle_of(oracle, small, rays)
    assert int(counts[0].min()) == int(counts[0].max()) == 30 and int(counts[1].sum()) == 1050
    assert np.count_nonzero(ref["image"]) == ref["image"].size
    two = run_plan(hip, small)
    lst = run_plan(hip, small, rays)
    assert not two["fused"] and two["failure_code"] == 0 and two["stats"]["cell_steps"] == ref["counters"]["cell_steps"]
    gate_outputs(two, ref, small, counts, TIGHT_TIER, "pairs c: backward seeded, 7 x 5 x 6 x 5 own grid against the oracle")
    gate_outputs(two, lst, small, counts, "reordering", "pairs c: backward seeded, own grid against the same rays as a list")
    monkeypatch.setenv("RT_HIP_FUSED_SEED", "1")
    one = run_plan(hip, small)
    monkeypatch.delenv("RT_HIP_FUSED_SEED")
    note(f"pairs c: backward seeded own grid under RT_HIP_FUSED_SEED=1, one launch taken: {one['fused']}")
    assert one["failure_code"] == 0 and one["stats"]["cell_steps"] == ref["counters"]["cell_steps"]
    gate_outputs(one, two, small, counts, "reordering", f"pairs c: RT_HIP_FUSED_SEED=1 (one launch {one['fused']}) against the two-kernel run")
    gate_outputs(one, ref, small, counts, TIGHT_TIER, f"pairs c: RT_HIP_FUSED_SEED=1 (one launch {one['fused']}) against the oracle")


# ---------------------------------------------------------------------------------------------- d. exact emission
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_exact_emission_forward_ase(hip, oracle, ase_small, seed_small, n):
    """el / gl per frequency as the CPU has them: a wrong slot order or offset of evl shows at rounding level here."""
    p = pair_problem("fwd_ase", ase_small, seed_small)
    rays = p.build_rays(list_ids("fwd_ase", n))
    against_the_oracle(hip, oracle, p, rays, f"pairs d: forward ASE, exact emission, {n} rays", exact=True)


# ---------------------------------------------------------------------------------------------- e. other N
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("pair", PAIRS)
def test_other_numbers_of_lengths(hip, oracle, ase_small, seed_small, pair, N):
    """N != 3: the instances with SF = 0; N = 5: the tables leave LDS and the global-table march runs."""
    p = with_lengths(pair_problem(pair, ase_small, seed_small), N)
    assert p.N == N and p.method == (2 if pair == "fwd_ase" else 1)
    rays = p.build_rays(mp.strided_ids(p, 397))
    _, ref, _ = against_the_oracle(hip, oracle, p, rays, f"pairs e: {pair}, N = {N}, every 397th ray")
    assert np.count_nonzero(ref["image"]) > 30000


# ---------------------------------------------------------------------------------------------- f. other K
@pytest.mark.parametrize("nv", [1, 5, 66])
@pytest.mark.parametrize("pair", PAIRS)
def test_other_frequency_counts(hip, oracle, ase_small, seed_small, pair, nv):
    p = problem_mod.resample_frequency(pair_problem(pair, ase_small, seed_small), nv)
    assert p.beam.nv == nv and p.method == (2 if pair == "fwd_ase" else 1)
    rays = p.build_rays(mp.strided_ids(p, 397))
    _, ref, _ = against_the_oracle(hip, oracle, p, rays, f"pairs f: {pair}, K = {nv}, every 397th ray")
    assert np.count_nonzero(ref["image"]) >= 700 * nv


def test_one_frequency_with_a_seed_forward(hip, oracle, seed_small):
    """The pair next door at K = 1: a seed's fifth table is a list of nv values, not an interpolated axis -- one entry is a
    complete table (rt_hip_plan_create asked for two on every axis)."""
    p = problem_mod.resample_frequency(seed_small, 1)
    assert p.method == 2 and len(p.seed.f[4]) == 1
    rays = p.build_rays(mp.strided_ids(p, 397))
    _, ref, _ = against_the_oracle(hip, oracle, p, rays, "pairs f: forward seeded, K = 1, every 397th ray")
    assert np.count_nonzero(ref["image"]) >= 700


# ---------------------------------------------------------------------------------------------- g. the y mirror, with emission
def two_sided(p, beam_too):
    """The gain grids of test_two_sided_y_grid_takes_the_unmirrored_branch (tests/test_gpu_edges.py); beam_too: the beam's y
    axis mirrored likewise, so that beam.y[0] < 0 and the forward deposit does not mirror either."""
    q = copy.copy(p)
    gains = [p.gain[0]]
    for g in p.gain[1:]:
        Nx, Ny, K = g.Nx, g.Ny, g.Nv
        y2 = np.concatenate([-g.y[::-1] - 1e-6, g.y])

        def mir(a, w=1):
            a = a.reshape(Ny, Nx * w)
            return np.concatenate([a[::-1], a], axis=0).reshape(-1)

        gains.append(rt.Gain(g.x, y2, mir(g.n), mir(g.g0), mir(g.E0), mir(g.gv, K), K))
    q.gain = gains
    if beam_too:
        b = copy.copy(p.beam)
        b.y = np.concatenate([-p.beam.y[::-1], p.beam.y])
        assert np.allclose(np.diff(b.y), b.dy, rtol=1e-9)
        q.beam = b
    return q


@pytest.mark.parametrize("case", ["shipped_mirrored", "two_sided_gain_mirrored", "two_sided_not_mirrored"])
def test_y_mirror_of_the_forward_deposit_with_emission(hip, oracle, ase_small, seed_small, case):
    base = pair_problem("fwd_ase", ase_small, seed_small)
    if case == "shipped_mirrored":
        p = base
        rays = p.build_rays(mp.strided_ids(p, 101))
    else:
        p = two_sided(base, beam_too=case == "two_sided_not_mirrored")
        rays = base.build_rays(mp.strided_ids(base, 101))     # (the launch grid of the shipped beam ...)
        rays["y"][::2] *= -1                                  # (... every other ray from the lower half)
    assert (p.beam.y[0] >= 0) == (case != "two_sided_not_mirrored")
    ray2, err = oracle.exit_rays(p, rays)
    below = int(((ray2["y"] < 0) & (err == 0)).sum())
    note(f"pairs g: {case}: {below} of {len(rays)} rays leave with y < 0; beam.y[0] = {p.beam.y[0]:.3g}")
    assert 10 * below >= len(rays)
    out, ref, counts = against_the_oracle(hip, oracle, p, rays, f"pairs g: forward ASE, {case}")
    if case == "two_sided_not_mirrored":      # the lower half of the image is reached, and only without the mirror
        ny = p.beam.ny
        lower = ref["image"].reshape(ny, -1)[: ny // 2]
        assert np.count_nonzero(lower) > 1000 and int(counts[0].reshape(ny, -1)[: ny // 2].sum()) >= below // 2


# ---------------------------------------------------------------------------------------------- h. failure codes
def failing_cases(pair, p):
    """As test_failure_codes_match_the_cpu_loop (tests/test_gpu_edges.py) builds them: dict(name -> (problem, rays, bit)).
    In the gain-only mode a sign-flipped lineshape leaves Iv = seed x exp(.) non-negative (the CPU loop reports nothing),
    so error -2 of the seeded pair comes from negative entries of the seed's frequency profile, as tests/test_gpu_seed_set.py
    has it (a negative spatial factor is clipped to zero and fails nothing): every ray with a non-zero factor fails then; the sign-flipped row stays in as a clean case."""
    rays = p.build_rays(mp.strided_ids(p, 997 if pair == "fwd_ase" else 7803 * 4 + 1))
    bad = rays.copy()
    bad["a"][7] = 1500.0                       # error -1: almost perpendicular to z (Helper.h:515)
    bad["x"][9] = 10.0                         # outside the plasma from the start: no error, nothing amplified
    g = p.gain[2]
    gv = g.gv.copy().reshape(g.Ny, g.Nx, g.Nv)
    gv[:, :g.Nx // 2, 5] = np.nan              # (half of the table: the other rays stay clean and the repeat has something to show)
    gv = gv.reshape(-1)
    nan_p, neg_p = copy.copy(p), copy.copy(p)
    nan_p.gain = p.gain[:2] + [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, gv, g.Nv)]
    neg_p.gain = p.gain[:2] + [rt.Gain(g.x, g.y, g.n, g.g0, g.E0, -np.abs(g.gv), g.Nv)]
    cases = dict(invalid_and_outside=(p, bad, 1 << 1), nan_lineshape=(nan_p, rays, 1 << 3),
                 negative_lineshape=(neg_p, rays, (1 << 2) if pair == "fwd_ase" else 0))
    if pair == "bwd_seed":
        f4 = p.seed.f[4].copy()
        f4[1::3] = -np.abs(f4[1::3])
        q = copy.copy(p)
        q.seed = rt.Seed(list(p.seed.x), list(p.seed.f[:4]) + [f4], p.seed.f0)
        cases["negative_seed_profile"] = (q, rays, 1 << 2)
    return cases


@pytest.mark.parametrize("pair,case", [(pair, case) for pair in PAIRS for case in ("invalid_and_outside", "nan_lineshape", "negative_lineshape")]
                         + [("bwd_seed", "negative_seed_profile")])
def test_failure_codes(hip, oracle, ase_small, seed_small, pair, case):
    p, rays, bit = failing_cases(pair, pair_problem(pair, ase_small, seed_small))[case]
    ref = oracle.image_loop(p, rays)
    err = np.asarray(oracle.exit_rays(p, rays)[1])
    note(f"pairs h: {pair}, {case}: oracle failure code {ref['failure_code']}, rays per return code "
         f"{ {c: int((err == c).sum()) for c in (0, -1, -2, -3)} } of {len(rays)}")
    assert ref["failure_code"] == bit
    assert p.method == (2 if pair == "fwd_ase" else 1)
    out = run_plan(hip, p, rays)
    loop = hip.image_loop(p, rays)              # (staged outputs, then the checking repeat: the stale ones must not come back)
    for o, what in ((out, "plan"), (loop, "rt_hip_image_loop")):
        assert o["failure_code"] == ref["failure_code"], what
        assert len(o["failed_rays"]) == min(int((err != 0).sum()), rt.cabi.RT_N_FAILED_MAX), what
        failing = _ray_set(rays[err != 0])
        assert all(r in failing for r in _ray_set(o["failed_rays"])), what
        assert o["stats"]["cell_steps"] == ref["counters"]["cell_steps"], what
        if case in ("invalid_and_outside",) or bit == 0:     # non-negative inputs: the element gate, failing rays not counted
            if case == "invalid_and_outside":
                assert len(o["failed_rays"]) == 1 and o["failed_rays"][0] == rays[7] and err[9] == 0
            gate_outputs(o, ref, p, counts_from_oracle(oracle, p, rays), tier_of(p), f"pairs h: {pair}, {case}, {what} against the oracle")
        else:       # NaN and sign-flipped inputs are outside the element gate: the whole-array rule of a failing run
            same_outputs_in_a_failing_run(o, ref)
            if case != "negative_seed_profile":      # the clean rays of the repeat leave something to compare
                assert np.isfinite(ref["image"]).any() and ref["image"][np.isfinite(ref["image"])].any()


# ---------------------------------------------------------------------------------------------- i. spectra
def spectra_rays(pair, p):
    """200 rays of the grid, one invalid (error -1) and one that starts outside the plasma."""
    rays = p.build_rays(mp.strided_ids(p, p.n_rays_total // 200 + 1)[:200])
    assert len(rays) == 200
    rays["a"][5] = 1500.0
    rays["x"][9] = 10.0
    return rays


@pytest.mark.parametrize("pair", PAIRS)
def test_spectra(hip, oracle, ase_small, seed_small, pair):
    p = pair_problem(pair, ase_small, seed_small)
    m = p.method
    base = ase_small if pair == "fwd_ase" else seed_small      # (calc_rays is handed the method beside the problem)
    rays = spectra_rays(pair, p)
    ref = oracle.probe(p, rays)
    assert ref["err"][5] == -1 and ref["err"][9] == 0 and (ref["flags"][9] & 1) and int((ref["err"] == 0).sum()) == 199
    assert ref["Iv"].any(axis=1).sum() >= 100
    with hip.Plan(p) as plan:
        out = plan.set_rays(rays).enable_spectra().run().fetch_spectra()
        st = plan.fetch()
        exact = plan.set_exact_emission(True).run().fetch_spectra() if p.use_emis else None
    assert st["failure_code"] == 1 << 1 and len(st["failed_rays"]) == 1 and st["failed_rays"][0] == rays[5]
    check_against(out, ref, f"pairs i: {pair}, spectra of a plan against the oracle's probe")
    if exact is not None:
        check_against(exact, ref, f"pairs i: {pair}, spectra of a plan, exact emission, against the oracle's probe")
    by_call = hip.calc_rays(base, rays, method=m)
    check_against(by_call, ref, f"pairs i: {pair}, rt_hip_calc_rays with method {m} against the oracle's probe")
    other = hip.calc_rays(base, rays)
    assert not np.array_equal(other["Iv"], by_call["Iv"]), "calc_rays ignores its method"
    # the reference's own calc_ray on the first 200 of every 97th ray
    fx = np.load(GOLDEN / FIXTURE[pair])
    n = fx["Iv"].shape[0]
    rays = p.build_rays(mp.strided_ids(p, 97)[:n])
    want = dict(err=fx["err"].astype(np.int32), Iv=fx["Iv"], ray2=rt.cabi.rays_from_array(fx["ray2"]))
    assert n == 200 and not fx["err"].any()
    with hip.Plan(p) as plan:
        out = plan.set_rays(rays).enable_spectra().run().fetch_spectra()
    rows, nzero = check_against(out, want, f"pairs i: {pair}, spectra of a plan against the reference's calc_ray")
    assert rows + nzero == n
    rows, nzero = check_against(hip.calc_rays(base, rays, method=m), want, f"pairs i: {pair}, rt_hip_calc_rays against the reference's calc_ray")
    assert rows + nzero == n


# ---------------------------------------------------------------------------------------------- j. path tracer
@pytest.mark.parametrize("pair", PAIRS)
def test_path_tracer(hip, oracle, ase_small, seed_small, pair):
    p = pair_problem(pair, ase_small, seed_small)
    base = ase_small if pair == "fwd_ase" else seed_small
    fx = np.load(GOLDEN / FIXTURE[pair])
    ids, sub = mp.path_sub_grid(p, fx)
    xr, yr, Ir, nerr = hip.calc_ray_path(base, *sub, method=p.method, c=0.5)
    assert nerr == int(fx["nerr_path"])
    assert np.array_equal(xr.view(np.uint32), fx["x_path"].view(np.uint32))
    assert np.array_equal(yr.view(np.uint32), fx["y_path"].view(np.uint32))
    assert float(np.abs(fx["I_path"]).max()) > 0
    worst = float(np.max(np.abs(Ir - fx["I_path"]) / np.where(fx["I_path"] != 0, np.abs(fx["I_path"]), 1.0)))
    note(f"pairs j: {pair}, calc_ray_path against the reference's: positions bit-equal, worst relative intensity difference {worst:.3e}, gate 2e-06")
    assert np.allclose(Ir, fx["I_path"], rtol=2e-6, atol=0)
    want = oracle.calc_ray_path(p, p.build_rays(ids), 0.5)
    N2 = want["x"].shape[1]
    lay = lambda v: np.ascontiguousarray(v.reshape(*fx["n"], N2).transpose(3, 2, 1, 0, 4))
    assert np.array_equal(xr.view(np.uint32), lay(want["x"]).view(np.uint32)) and np.array_equal(yr.view(np.uint32), lay(want["y"]).view(np.uint32))
    assert np.allclose(Ir, lay(want["I"]), rtol=2e-6, atol=0)
    other = hip.calc_ray_path(base, *sub, c=0.5)[2]
    assert not np.array_equal(other, Ir), "calc_ray_path ignores its method"
    # a list with one failing and one escaped ray, through a plan
    rays = p.build_rays(mp.strided_ids(p, 331 if pair == "fwd_ase" else 331 * 20 + 1))
    rays["a"][5] = 1500.0      # error -1
    rays["x"][9] = 10.0        # outside the plasma from the start
    with hip.Plan(p) as plan:
        got = plan.enable_path().set_rays(rays).run().fetch_path()
    want = oracle.calc_ray_path(p, rays)
    assert np.array_equal(got["err"], want["err"]) and got["err"][5] == -1 and got["err"][9] == 0
    assert np.array_equal(got["x"].view(np.uint32), want["x"].view(np.uint32))
    assert np.array_equal(got["y"].view(np.uint32), want["y"].view(np.uint32))
    assert np.allclose(got["I"], want["I"], rtol=2e-6, atol=0) and np.abs(want["I"]).max() > 0


# ---------------------------------------------------------------------------------------------- k. step mode
def step_against_cubes(hip, oracle, p, rays, label, monkeypatch):
    """own_cube_and_oracle of tests/test_gpu_step.py with the counts taken from explicit rays (rays None: the ray grid on
    the device, its list for the oracle and the counts)."""
    img, step, info = image_then_step(hip, p, rays, monkeypatch)
    lst = p.build_rays() if rays is None else rays
    ora, counts = oracle_of(oracle, p, lst)
    assert info["failure_code"] == img["failure_code"] == ora["failure_code"] == 0, label
    assert info["stats"]["cell_steps"] == img["stats"]["cell_steps"] == ora["counters"]["cell_steps"], label
    gate_step(step, reduced(hip, p, img), p, counts, "reordering", f"{label} / step against the plan's own cube")
    gate_step(step, reduced(hip, p, ora), p, counts, tier_of(p), f"{label} / step against the oracle's cube")
    assert step["E_v"].any() and step["nf"].any() and step["I_ang"].any()
    return step, counts, ora


@pytest.mark.parametrize("pair", PAIRS)
def test_step_mode(hip, oracle, ase_small, seed_small, pair, monkeypatch):
    """E_v, nf and I_ang against the reduction of the plan's own cube (reordering) and of the oracle's (the tier), on the
    grid of (b) and on a list; rt_hip_step_loop likewise."""
    p = grid_problem(pair, ase_small, seed_small)
    step, counts, ora = step_against_cubes(hip, oracle, p, None, f"pairs k: {pair}, grid of (b)", monkeypatch)
    full = pair_problem(pair, ase_small, seed_small)
    rays = full.build_rays(mp.strided_ids(full, 397))
    lst, lcounts, _ = step_against_cubes(hip, oracle, full, rays, f"pairs k: {pair}, every 397th ray", monkeypatch)
    loop = hip.step_loop(full, rays)
    assert loop["failure_code"] == 0 and loop["stats"]["n_rays"] == len(rays)
    gate_step(loop, lst, full, lcounts, "reordering", f"pairs k: {pair}, rt_hip_step_loop against the plan")
    if pair != "fwd_ase":
        return
    # forward ASE with the one launch asked for: it must stay on two kernels and give the same record
    monkeypatch.delenv("RT_HIP_FUSED", raising=False)
    back = mp.with_method(p, 1)
    with hip.Plan(back) as plan:
        plan.set_ray_grid().enable_step().set_step_one_launch(True).run()
        plan.fetch_step()
        assert plan.last_fused(), "the control (method 1) did not take the one launch: this grid no longer shows what it is meant to show"
    with hip.Plan(p) as plan:
        plan.set_ray_grid().enable_step().set_step_one_launch(True).run()
        asked = plan.fetch_step()
        info = plan.fetch()
        fused = plan.last_fused()
    note(f"pairs k: forward ASE with set_step_one_launch(True), one launch taken: {fused} (backward on the same grid: True)")
    assert not fused and info["failure_code"] == 0
    gate_step(asked, step, p, counts, "reordering", "pairs k: forward ASE, one launch asked for, against the plain step run")
    gate_step(asked, reduced(hip, p, ora), p, counts, tier_of(p), "pairs k: forward ASE, one launch asked for, against the oracle's cube")


# ---------------------------------------------------------------------------------------------- l. host-pointer and multi-device entries
@pytest.mark.parametrize("pair", PAIRS)
def test_host_pointer_entry_recognises_the_grid(hip, oracle, ase_small, seed_small, pair):
    p = grid_problem(pair, ase_small, seed_small)
    rays = p.build_rays()
    gx, gy, ga, gb = p.ray_grid
    assert hip.ray_list_grid_dims(rays) == (len(gx), len(gy), len(ga), len(gb))
    ref, counts = oracle_of(oracle, p, rays)
    out = hip.image_loop(p, rays)
    plan = run_plan(hip, p)
    assert out["failure_code"] == 0 and out["stats"]["n_rays"] == len(rays) and out["stats"]["cell_steps"] == ref["counters"]["cell_steps"]
    gate_outputs(out, ref, p, counts, tier_of(p), f"pairs l: {pair}, rt_hip_image_loop on the grid of (b) against the oracle")
    gate_outputs(out, plan, p, counts, "reordering", f"pairs l: {pair}, rt_hip_image_loop against the plan's ray grid")


def test_multi_device_entry_sends_forward_ase_down_the_sum_reduce_path(hip, oracle, ase_small, seed_small, monkeypatch):
    """Pixel-column tiles would be wrong for a deposit at the exit ray: mode 2 (ray chunks + sum-reduce), two workers."""
    p = grid_problem("fwd_ase", ase_small, seed_small)
    rays = p.build_rays()
    ref, counts = oracle_of(oracle, p, rays)
    one = hip.image_loop(p, rays)
    monkeypatch.setenv("RT_HIP_MULTI_LOOPBACK", "2")
    out = hip.multi_image_loop(p, rays)
    back = hip.multi_image_loop(mp.with_method(p, 1), rays)
    monkeypatch.delenv("RT_HIP_MULTI_LOOPBACK")
    note(f"pairs l: multi-device entry, two loop-back workers: forward ASE mode {out['mode']}, backward ASE mode {back['mode']}")
    assert back["mode"] == 1, "the control (method 1 on the beam's own grid) did not take the pixel tiles"
    assert out["mode"] == 2
    assert out["failure_code"] == 0 and out["stats"]["n_rays"] == len(rays) and out["stats"]["cell_steps"] == one["stats"]["cell_steps"]
    gate_outputs(out, one, p, counts, "reordering", "pairs l: forward ASE, two loop-back workers against one device")
    gate_outputs(out, ref, p, counts, DEFAULT_TIER, "pairs l: forward ASE, two loop-back workers against the oracle")


# ---------------------------------------------------------------------------------------------- m. neither emission nor seed
@pytest.mark.parametrize("method", [1, 2])
def test_neither_emission_nor_seed(hip, oracle, ase_small, method):
    """Gain tables without E0 and no seed: nothing to amplify -- image and I_ang exactly zero under both methods, the march
    as the oracle's (the reference agrees: its Iv starts from zero)."""
    q = copy.copy(ase_small)
    q.gain = [rt.Gain(g.x, g.y, g.n, g.g0, None, g.gv, g.Nv) for g in ase_small.gain]
    p = mp.with_method(q, method)
    assert not p.use_emis and p.seed is None
    rays = p.build_rays(mp.strided_ids(p, 997))
    ref = oracle.image_loop(p, rays)
    assert ref["failure_code"] == 0 and not ref["image"].any() and not ref["I_ang"].any()
    out = run_plan(hip, p, rays, probe=True)
    same_record(out["probe"], oracle.probe(p, rays, want_Iv=False))
    assert out["failure_code"] == 0 and len(out["failed_rays"]) == 0
    assert out["stats"]["cell_steps"] == ref["counters"]["cell_steps"] > 0
    assert not out["image"].any() and not out["I_ang"].any()
    assert np.array_equal(out["image"], ref["image"]) and np.array_equal(out["I_ang"], ref["I_ang"])
    # the other two passes read the same (absent) frequency profile
    with hip.Plan(p) as plan:
        sp = plan.set_rays(rays).enable_spectra().run().fetch_spectra()
        assert plan.fetch()["failure_code"] == 0
        step = plan.enable_spectra(False).enable_step().run().fetch_step()
    assert not sp["err"].any() and not sp["Iv"].any() and sp["Iv"].shape == (len(rays), p.beam.nv)
    assert not step["E_v"].any() and not step["nf"].any() and not step["I_ang"].any()
